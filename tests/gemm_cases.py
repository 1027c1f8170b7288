"""The split-K / persistent-loop cases of gemm_kernel (csrc/gemm_conv.hip), shared by tests/test_gemm_dispatch_cpu.py (which
pins the variant the library reports for each: no GPU) and the GPU tests that run them (tests/test_gemm_splitk_gpu.py,
tests/test_fp8_gpu.py::test_gemm_fp8).

A work item of the kernel is (output tile x K split).  Tiles are ``rows`` x 160 (rows = 64 or 128 for the bf16 GEMM, 128 for
fp8 and the implicit-GEMM conv); split s of S covers the K tiles [KT s // S, KT (s + 1) // S) of KT = K / 64 (fp8: K / 128:
a K tile is 128 bytes of a row).  The grid is min(items, 512) persistent workgroups: workgroup g takes the items
perm(g), perm(g) + grid, ... where perm is the kernel's XCD map, whose ``r != 0`` branch runs when grid % 8 != 0.

Every case carries the variant it is meant to hit (rows / split / items / K tiles per split) and the properties it exists
for; ``derive`` computes the numbers and ``holds`` decides a property from them alone.  If a retune of sd_gemm_tile_rows /
sd_gemm_splitk moves a case, the CPU test fails: change the SHAPE until its properties hold again."""
from collections import namedtuple

BN = 160                    # tile columns
PERSISTENT_GRID = 512       # 2 workgroups per CU x 256 CUs (csrc/gemm_conv.hip::kPersistentGrid)

# what gemm_kernel does differently when a property holds
PROPS = {
    "rows == 64": "the 64-row tile (waves own 32 rows)",
    "split > 1": "partials go to fp32 slabs, splitk_reduce_kernel finishes",
    "m_tiles >= 2": "a split's slab holds more than one row tile",
    "M % rows != 0": "zero-page rows and dropped slab rows in the last M tile",
    "N % 160 != 0": "a partial last N tile",
    "grid % 8 != 0": "the r != 0 branch of the XCD map",
    "items > 512": "a workgroup takes a second item, with another kt_begin, prefetched before its epilogue",
    "K1 inside a split": "one split reads K tiles of both segments (X, then X2)",
    "splits uneven": "KT is not a multiple of the split factor",
}

GemmCase = namedtuple("GemmCase", "M N K K1 bias bias2 res rows split items kts props why")
ConvCase = namedtuple("ConvCase", "B H W Cin Cout stride bias2 res rows split items kts props why")
Fp8Case = namedtuple("Fp8Case", "M N K bias res rows split items kts props why")

# ---- bf16 GEMM through sd_op_gemm (K1 == K: one segment) ------------------------------------------------------------
GEMM_CASES = [
    GemmCase(77, 768, 3072, 3072, True, False, True, 64, 4, 40, (12, 12, 12, 12),
             ("rows == 64", "split > 1", "m_tiles >= 2", "M % rows != 0", "N % 160 != 0"),
             "CLIP text fc2, one prompt: M tail 13, N tail 128"),
    GemmCase(257, 1024, 4096, 4096, True, False, True, 64, 5, 175, (12, 13, 13, 13, 13),
             ("rows == 64", "split > 1", "m_tiles >= 2", "M % rows != 0", "N % 160 != 0", "grid % 8 != 0", "splits uneven"),
             "ViT-L/14 fc2, one image: uneven splits, grid % 8 = 7, N tail 64, M tail 1"),
    GemmCase(128, 1280, 5120, 5120, True, False, True, 64, 6, 96, (13, 13, 14, 13, 13, 14),
             ("rows == 64", "split > 1", "m_tiles >= 2", "splits uneven"),
             "ff.net.2 of the 8x8 level, UNet batch 2: two full 64-row tiles, 13/13/14 splits"),
    GemmCase(514, 1280, 5120, 5120, True, False, False, 64, 6, 432, (13, 13, 14, 13, 13, 14),
             ("rows == 64", "split > 1", "m_tiles >= 2", "M % rows != 0", "splits uneven"),
             "ViT-H fc2, two images: 9 M tiles, M tail 2"),
    GemmCase(192, 1280, 2560, 1280, True, True, True, 64, 3, 72, (13, 13, 14),
             ("rows == 64", "split > 1", "m_tiles >= 2", "K1 inside a split", "splits uneven"),
             "two K segments: K1 at tile 20 inside split 1 (tiles 13..25)"),
    GemmCase(192, 640, 1920, 1280, False, False, True, 64, 2, 24, (15, 15),
             ("rows == 64", "split > 1", "m_tiles >= 2", "K1 inside a split"),
             "K1 inside split 1, second segment shorter than the first"),
    GemmCase(200, 324, 1536, 1536, True, False, False, 64, 2, 24, (12, 12),
             ("rows == 64", "split > 1", "m_tiles >= 2", "M % rows != 0", "N % 160 != 0"),
             "N tail of 4 columns, M tail 8"),
    GemmCase(3072, 640, 2560, 2560, True, False, True, 64, 3, 576, (13, 13, 14),
             ("rows == 64", "split > 1", "m_tiles >= 2", "items > 512", "splits uneven"),
             "ff.net.2 of the 32x32 level, UNet batch 3: the persistent loop on the 64-row tile"),
    GemmCase(3000, 640, 2560, 2560, True, True, False, 64, 3, 564, (13, 13, 14),
             ("rows == 64", "split > 1", "m_tiles >= 2", "M % rows != 0", "items > 512", "splits uneven"),
             "the same with an M tail of 56 rows in the last tile"),
    GemmCase(6144, 1280, 1536, 1536, True, False, True, 128, 2, 768, (12, 12),
             ("split > 1", "m_tiles >= 2", "items > 512"),
             "the persistent loop on the 128-row tile"),
]
GEMM_PITCHED = (0, 4)               # the cases that also run with pitched ldx / ldx2 / ldr / ldc
GEMM_DETERMINISM = 7                # launched twice: the split-K finish is deterministic

# The case of the fault demonstrations in tests/test_bounds_cpu.py (also run on the GPU).  One N tile, 170 M tiles, an M tail
# of ONE row, three splits of which the second straddles K1 (tile 20 of 13..25) and the third lies wholly in the second
# segment: see that file for why a fault has to be this diluted to pass a whole-tensor norm.
FAULT_CASE = GemmCase(10817, 160, 2560, 1280, True, False, True, 64, 3, 510, (13, 13, 14),
                      ("rows == 64", "split > 1", "m_tiles >= 2", "M % rows != 0", "grid % 8 != 0", "K1 inside a split",
                       "splits uneven"),
                      "170 M tiles of one N tile, M tail 1, K1 inside split 1")

# ---- implicit-GEMM 3x3 conv through sd_op_conv3x3 (stride 2: never the halo kernel; bias always) -----------------------
CONV_CASES = [
    ConvCase(2, 64, 64, 320, 320, 2, True, True, 128, 3, 96, (15, 15, 15),
             ("split > 1", "m_tiles >= 2"),
             "the UNet's first downsampler at UNet batch 2: 16 M tiles x 2 N tiles"),
    ConvCase(4, 128, 128, 192, 480, 2, False, False, 128, 2, 768, (13, 14),
             ("split > 1", "m_tiles >= 2", "items > 512", "splits uneven"),
             "the persistent loop with AMODE_CONV: the next item's prefetch crosses image and split boundaries"),
]

# ---- fp8 GEMM through sd_op_gemm_fp8 (appended to test_gemm_fp8's own list) --------------------------------------------
FP8_CASES = [
    Fp8Case(300, 1280, 5120, True, True, 128, 3, 72, (13, 13, 14),
            ("split > 1", "m_tiles >= 2", "M % rows != 0", "splits uneven"), "3 M tiles, M tail 44"),
    Fp8Case(257, 1024, 4096, True, False, 128, 2, 42, (16, 16),
            ("split > 1", "m_tiles >= 2", "M % rows != 0", "N % 160 != 0", "grid % 8 != 0"), "N tail 64, M tail 1"),
    Fp8Case(6144, 1280, 3072, False, True, 128, 2, 768, (12, 12),
            ("split > 1", "m_tiles >= 2", "items > 512"),
            "the persistent loop with the dequantisation in splitk_reduce_kernel"),
]


def conv_dims(c):
    """(M, N, K, Hout, Wout) of a ConvCase (3x3, padding 1)."""
    Ho, Wo = (c.H + 2 - 3) // c.stride + 1, (c.W + 2 - 3) // c.stride + 1
    return c.B * Ho * Wo, c.Cout, 9 * c.Cin, Ho, Wo


def mnk(c):
    return conv_dims(c)[:3] if isinstance(c, ConvCase) else (c.M, c.N, c.K)


def k_tile(c):
    """K elements per K tile: 128 bytes of an operand row."""
    return 128 if isinstance(c, Fp8Case) else 64


def split_ranges(KT, split):
    """[kt_begin, kt_end) of every split, as gemm_kernel's decode() computes them."""
    return [(KT * s // split, KT * (s + 1) // split) for s in range(split)]


def derive(c, rows, split):
    """The numbers the properties are decided from, for the (rows, split) the library reports."""
    M, N, K = mnk(c)
    m_tiles, n_tiles = -(-M // rows), -(-N // BN)
    items = m_tiles * n_tiles * split
    ranges = split_ranges(K // k_tile(c), split)
    return dict(M=M, N=N, K=K, rows=rows, split=split, m_tiles=m_tiles, n_tiles=n_tiles, items=items,
                grid=min(items, PERSISTENT_GRID), ranges=ranges, kts=tuple(e - b for b, e in ranges),
                k1_tile=getattr(c, "K1", K) // k_tile(c))


def holds(prop, d):
    """Whether property ``prop`` (a key of PROPS) holds for the numbers of derive()."""
    if prop == "rows == 64":
        return d["rows"] == 64
    if prop == "split > 1":
        return d["split"] > 1
    if prop == "m_tiles >= 2":
        return d["m_tiles"] >= 2
    if prop == "M % rows != 0":
        return d["M"] % d["rows"] != 0
    if prop == "N % 160 != 0":
        return d["N"] % BN != 0
    if prop == "grid % 8 != 0":           # (items % 8 != 0 with every item its own workgroup: the grid is what the map sees)
        return d["grid"] % 8 != 0 and d["items"] % 8 != 0
    if prop == "items > 512":
        return d["items"] > PERSISTENT_GRID
    if prop == "K1 inside a split":
        return any(b < d["k1_tile"] < e for b, e in d["ranges"])
    if prop == "splits uneven":
        return len(set(d["kts"])) > 1
    raise KeyError(prop)


def case_id(c):
    if isinstance(c, ConvCase):
        return f"conv{c.B}x{c.H}x{c.W}-{c.Cin}to{c.Cout}-s{c.stride}"
    M, N, K = mnk(c)
    return f"{M}x{N}x{K}" + (f"-K1_{c.K1}" if getattr(c, "K1", K) != K else "")
