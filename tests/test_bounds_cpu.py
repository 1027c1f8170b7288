"""The elementwise gate of tests/bounds.py, checked without a GPU.

Exact fp64 results rounded to the output format stand in for a correct kernel: they must pass with margin.  Faults of the
kinds the kernels risk (a halo corner, a wrapped halo column, a dropped bias, a split-K slab counted twice, a ragged key
tile, a tail row from the neighbouring image; on a split-K GEMM of 170 row tiles: a tile that counts a split twice, an item that
starts one K tile late, tail rows with the residual of another row, a second K segment read from the wrong offset) are injected
into the same results: each must pass the rel-L2 gate the GPU
tests have always used -- the gap is real -- and fail the elementwise gate.  The guard bands must catch single stray
stores and accept an untouched buffer.

The flip budget (assert_flip_budget) is checked the same way for GroupNorm: every fp32 restatement passes against the
others, an eps 10x / 100x too large and a count off by one fail it at a small-kernel shape and at (1, 1024, 1280), for bf16
and for e4m3 outputs -- and eps x 100 (bf16) / eps = 1e-3 (e4m3) still pass the per-element gates, which is the gap the
budget closes.  Measured here (flips of numel, restatement form 0 as "the kernel"):
    bf16 (1, 256, 1280) 327680:   F_ref 33;  eps x 10 1372, eps x 100 10895, cnt + 1 5516
    bf16 (1, 1024, 1280) 1310720: F_ref 208; eps x 10 5188, eps x 100 42016, cnt + 1 6415
    e4m3 (1, 256, 1280) x 8:      F_ref 1;   eps x 10 47,   eps = 1e-3 629,   cnt + 1 528
    e4m3 (1, 1024, 1280) x 8:     F_ref 21;  eps x 10 230,  eps = 1e-3 2595,  cnt + 1 558
(F_ref: 48 .. 54 with torch's pairwise sums, 206 .. 208 with serial sums over the pixels at 1024 x 40 values per group.)
At 64 pixels x 20 channels per group the statistics term of the e4m3 gate is small enough to refuse eps = 1e-3 on 4 of 161
differing codes; from 10240 values per group on it passes it whole."""
import math

import pytest
import torch
import torch.nn.functional as F

from tests.bounds import (U32, assert_e4m3_codes, assert_e4m3_interval, assert_elementwise, assert_flip_budget, attention_ref_bound, check_guards,
                          conv3x3_nhwc_ref, count_flips, elementwise_ratio, flip_ordinals, forget_guards, gemm_bound,
                          gn_restatements, guarded, guarded_input, linear_bound, ln_restatements, near_midpoint_count,
                          norm_ref_bound, ulp_bf16, ulp_e4m3)
from tests.util import rel_l2

OLD_TOL, OLD_TOL_ATTN = 6e-3, 1e-2


def r16(t):
    return t.to(torch.bfloat16).double()


def worst_ratio(got, ref, bound):
    return float(elementwise_ratio(got, ref, bound)[2].max())


def fault_report(name, got, ref, bound, old_tol, old_gate_passes=True):
    e, w = rel_l2(got, ref), worst_ratio(got, ref, bound)
    print(f"fault {name}: rel-L2 {e:.2e} (old gate {old_tol:g}), worst err/bound {w:.2f}")
    if old_gate_passes:
        assert e < old_tol, f"{name}: the old gate already catches this fault"
    assert w > 1.0, f"{name}: the elementwise gate misses this fault"
    with pytest.raises(AssertionError):
        assert_elementwise(got, ref, bound, f"fault {name}")


# ---- conv 2 x 64 x 64, 320 -> 320 -------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def conv64():
    g = torch.Generator().manual_seed(1)
    B, H, C = 2, 64, 320
    x = r16(torch.randn(B, C, H, H, generator=g))
    w = r16(torch.randn(C, C, 3, 3, generator=g) / math.sqrt(9 * C))
    b = torch.randn(C, generator=g).double() * 0.05
    ref, mag = conv3x3_nhwc_ref(x, w, b)
    bound = linear_bound(ref, mag, 9 * C + 3)
    return x, w, b, ref, bound, r16(ref)


def tap(x, w, b_, y, xx, dy, dx):
    """The contribution of tap (dy, dx) to output pixel (b_, y, xx), all output channels, reading input pixel
    (y + dy - 1, xx + dx - 1) -- wherever the caller says that lands."""
    return w[:, :, dy, dx] @ x[b_, :, y, xx]


def test_exact_conv_passes_with_margin(conv64):
    _, _, _, ref, bound, out = conv64
    w = assert_elementwise(out, ref, bound, "exact conv 2x64x64 320->320", ("b", "y", "x", "c"))
    assert w <= 0.5 + 1e-9


def test_exact_geometry_mode_conv_passes_with_margin():
    g = torch.Generator().manual_seed(2)
    B, H, W, C = 32, 7, 9, 320
    x = r16(torch.randn(B, C, H, W, generator=g))
    w = r16(torch.randn(C, C, 3, 3, generator=g) / math.sqrt(9 * C))
    b = torch.randn(C, generator=g)
    ref, mag = conv3x3_nhwc_ref(x, w, b)
    assert assert_elementwise(r16(ref), ref, linear_bound(ref, mag, 9 * C + 3), "exact conv 32x7x9 320->320",
                              ("b", "y", "x", "c")) <= 0.5 + 1e-9


def test_fault_corner_pixel_misses_its_centre_tap(conv64):
    x, w, _, ref, bound, _ = conv64
    bad = ref.clone()
    bad[1, 63, 63] -= tap(x, w, 1, 63, 63, 1, 1)
    fault_report("corner pixel misses its centre tap", r16(bad), ref, bound, OLD_TOL)


def test_fault_one_element_off_by_one(conv64):
    _, _, _, ref, bound, out = conv64
    bad = out.clone()
    bad[0, 17, 40, 100] += 1.0
    fault_report("one element +1.0", bad, ref, bound, OLD_TOL)


def test_fault_wrapped_halo_column(conv64):
    """Pixel (y, 0) reads its left neighbour from the end of the previous row instead of the zero padding."""
    x, w, _, ref, bound, _ = conv64
    bad = ref.clone()
    bad[0, 20, 0] += tap(x, w, 0, 19, 63, 1, 0)
    fault_report("wrapped halo column", r16(bad), ref, bound, OLD_TOL)


def test_fault_one_channel_bias_dropped(conv64):
    _, _, b, ref, bound, _ = conv64
    c = int(b.abs().argsort()[len(b) // 2])                   # a channel with a median bias
    bad = ref.clone()
    bad[..., c] -= b[c]
    fault_report("one channel's bias dropped", r16(bad), ref, bound, OLD_TOL)


def test_fault_splitk_slab_counted_twice(conv64):
    """One 16 x 16 accumulator tile adds the partial of input-channel slice 64..127 (all 9 taps) twice."""
    x, w, _, ref, bound, _ = conv64
    xs = F.pad(x[:, 64:128], (1, 1, 1, 1))
    slab = torch.zeros(2, 64, 64, 320, dtype=torch.float64)
    for dy in range(3):
        for dx in range(3):
            slab += torch.einsum("bchw,oc->bhwo", xs[:, :, dy:dy + 64, dx:dx + 64], w[:, 64:128, dy, dx])
    bad = ref.clone()
    bad[1, 40, 16:32, 160:176] += slab[1, 40, 16:32, 160:176]
    fault_report("split-K slab counted twice", r16(bad), ref, bound, OLD_TOL)


def test_fault_tail_row_from_the_neighbouring_image(conv64):
    """The last pixel of image 0 takes its lower halo row from image 1's first row instead of the zero padding."""
    x, w, _, ref, bound, _ = conv64
    bad = ref.clone()
    for dx in (0, 1):
        bad[0, 63, 63] += tap(x, w, 1, 0, 62 + dx, 2, dx)
    fault_report("tail row from the neighbouring image", r16(bad), ref, bound, OLD_TOL)


# ---- GEMM -------------------------------------------------------------------------------------------------------------

def test_gemm_tails_and_fault_last_row_misses_k_tail():
    g = torch.Generator().manual_seed(3)
    M, N, K = 1000, 960, 320
    x = r16(torch.randn(M, K, generator=g))
    w = r16(torch.randn(N, K, generator=g) / math.sqrt(K))
    b = torch.randn(N, generator=g)
    r = r16(torch.randn(M, N, generator=g))
    ref, bound = gemm_bound(x, w, b, None, r)
    assert assert_elementwise(r16(ref), ref, bound, "exact gemm 1000x960x320", ("row", "col")) <= 0.5 + 1e-9
    ref2, bound2 = gemm_bound(x, w)
    bad = ref2.clone()
    bad[-1] -= x[-1, -32:] @ w[:, -32:].t()
    fault_report("last row misses the last 32 of K", r16(bad), ref2, bound2, OLD_TOL, old_gate_passes=False)


# ---- split-K GEMM over many row tiles ---------------------------------------------------------------------------------
# Faults of gemm_kernel's work loop (csrc/gemm_conv.hip: decode(), the next item's prefetch, the K1 boundary inside a split)
# and of splitk_reduce_kernel, on tests/gemm_cases.py::FAULT_CASE: 10817 x 160 x 2560 with K1 = 1280, bias and residual; 64-row
# tiles, 170 M tiles of one N tile, the last tile holding ONE row; three splits over K tiles 0..12 | 13..25 | 26..39, K1 at
# tile 20 (tests/test_gemm_dispatch_cpu.py pins that variant).  The old gate is the 1e-2 rel-L2 of the whole-model tests, the
# only ones that ran these paths.
#
# Why this shape: a norm over the whole output sees a fault by its share of the energy.  With unit-variance product, bias
# and residual, a FULL 64 x 160 tile that counts one of S splits twice carries (10240 / (M N)) / (3 S) of it, and the
# heuristic gives S <= 512 x 10240 / (M N): rel-L2 >= sqrt(1 / (3 x 512)) = 2.6e-2 at every shape, above the old gate.  The
# faults that slip under it are those of a ragged last tile, of one K tile of one item, or of the few tail rows -- where such
# kernels go wrong -- and the shape is as large as a split-K problem gets so that a whole row of residuals from the wrong row
# (energy 2 N of 3 M N) stays below 1e-2 as well.  The full-tile forms are reported too: both gates refuse them.

GEMM_OLD_TOL = 1e-2


@pytest.fixture(scope="module")
def splitk_case():
    from tests.gemm_cases import FAULT_CASE as c, derive
    d = derive(c, c.rows, c.split)
    assert (d["m_tiles"], d["n_tiles"], d["M"] % c.rows, d["ranges"], d["k1_tile"]) == (170, 1, 1, [(0, 13), (13, 26), (26, 40)], 20)
    g = torch.Generator().manual_seed(12)
    x = r16(torch.randn(c.M, c.K, generator=g))
    w = r16(torch.randn(c.N, c.K, generator=g) / math.sqrt(c.K))
    b = torch.randn(c.N, generator=g).float().double()
    r = r16(torch.randn(c.M, c.N, generator=g))
    ref, bound = gemm_bound(x, w, b, None, r)
    return c, d, x, w, r, ref, bound


def partial(x, w, rows, kt0, kt1, xk0=None):
    """Rows ``rows`` of the partial product over K tiles [kt0, kt1); xk0: the K tile X is read from instead of kt0."""
    xk0 = kt0 if xk0 is None else xk0
    return x[rows, xk0 * 64:(xk0 + kt1 - kt0) * 64] @ w[:, kt0 * 64:kt1 * 64].t()


def test_exact_splitk_gemm_passes_with_margin(splitk_case):
    c, _, _, _, _, ref, bound = splitk_case
    assert assert_elementwise(r16(ref), ref, bound, f"exact gemm {c.M}x{c.N}x{c.K}", ("row", "col")) <= 0.5 + 1e-9


def test_fault_one_tile_adds_one_split_s_partial_twice(splitk_case):
    """(a) The last 64 x 160 tile (its one valid row) adds split 1's slab twice; the same on a full tile fails both gates."""
    c, d, x, w, _, ref, bound = splitk_case
    tail = slice(c.M - 1, c.M)
    bad = ref.clone()
    bad[tail] += partial(x, w, tail, *d["ranges"][1])
    fault_report("last tile adds split 1 twice", r16(bad), ref, bound, GEMM_OLD_TOL)
    full = slice(64, 128)
    bad = ref.clone()
    bad[full] += partial(x, w, full, *d["ranges"][1])
    fault_report("a full tile adds split 1 twice", r16(bad), ref, bound, GEMM_OLD_TOL, old_gate_passes=False)


def test_fault_second_m_tile_s_last_split_starts_one_k_tile_late(splitk_case):
    """(b) The item (M tile 1, last split) decodes kt_begin + 1: the 64-wide K tile 26 is missing from rows 64..127."""
    c, d, x, w, _, ref, bound = splitk_case
    kt = d["ranges"][-1][0]
    rows = slice(64, 128)
    bad = ref.clone()
    bad[rows] -= partial(x, w, rows, kt, kt + 1)
    fault_report("M tile 1, last split, starts one K tile late", r16(bad), ref, bound, GEMM_OLD_TOL)


def test_fault_tail_rows_take_the_residual_of_the_tile_above(splitk_case):
    """(c) The reduce adds R[m - rows] to the rows of the M tail (a clamped or tile-relative row index)."""
    c, _, _, _, r, ref, bound = splitk_case
    first = c.M - c.M % c.rows
    bad = ref.clone()
    bad[first:] += r[first - c.rows:c.M - c.rows] - r[first:]
    fault_report("tail rows with the residual of row m - 64", r16(bad), ref, bound, GEMM_OLD_TOL)


def test_fault_second_segment_read_from_the_wrong_offset(splitk_case):
    """(d) The K1 boundary inside a split, on the last tile's items.  Split 1 straddles it: its X2 tiles 20..25 are X2's first
    six, and a kernel that indexes X2 by the tile's position in the SPLIT reads tiles 7..12 of X2 instead.  Split 2 lies wholly
    in the second segment: reading 'from X2's start' instead of from its offset gives it X2 tiles 0..13 for 6..19."""
    c, d, x, w, _, ref, bound = splitk_case
    tail = slice(c.M - 1, c.M)
    (b1, e1), (b2, e2) = d["ranges"][1], d["ranges"][2]
    k1 = d["k1_tile"]
    assert b1 < k1 < e1 and b2 > k1
    bad = ref.clone()
    bad[tail] += partial(x, w, tail, k1, e1, xk0=k1 + (k1 - b1)) - partial(x, w, tail, k1, e1)
    fault_report("the straddling split indexes X2 by the position in the split", r16(bad), ref, bound, GEMM_OLD_TOL)
    bad = ref.clone()
    bad[tail] += partial(x, w, tail, b2, e2, xk0=k1) - partial(x, w, tail, b2, e2)
    fault_report("the split behind it reads X2 from its start", r16(bad), ref, bound, GEMM_OLD_TOL)


# ---- attention --------------------------------------------------------------------------------------------------------

def test_attention_4096_and_fault_ragged_last_key_tile():
    g = torch.Generator().manual_seed(4)
    B, H, N, D = 2, 1, 4096, 40
    q, k, v = (r16(torch.randn(B, H, N, D, generator=g)) for _ in range(3))
    scale = 1.0 / math.sqrt(D)
    ref, bound = attention_ref_bound(q, k, v, scale)
    assert assert_elementwise(r16(ref), ref, bound, "exact attention 2x4096x4096 d40", ("b", "head", "row", "d")) <= 0.5 + 1e-9
    bad = ref.clone()
    rows = slice(1000, 1016)
    s = (q[1, 0, rows] @ k[1, 0, :N - 64].t()) * scale
    bad[1, 0, rows] = torch.softmax(s, -1) @ v[1, 0, :N - 64]
    fault_report("16 query rows lose the last 64-key tile", r16(bad), ref, bound, OLD_TOL_ATTN)


# ---- GroupNorm, e4m3 --------------------------------------------------------------------------------------------------

def test_exact_groupnorm_passes_and_one_group_off():
    g = torch.Generator().manual_seed(5)
    B, HW, C = 2, 1024, 640
    x = r16(torch.randn(B, HW, C, generator=g) * 2 + 0.5)
    gamma, beta = torch.randn(C, generator=g), torch.randn(C, generator=g)
    ref, bound = norm_ref_bound(x, gamma, beta, HW * C // 32, 1e-5, True, groups=32)
    assert assert_elementwise(r16(ref), ref, bound, "exact groupnorm 2x1024x640", ("b", "pixel", "c")) <= 0.5 + 1e-9
    bad = ref.clone()                                   # one pixel's group normalised with a 1% wrong rstd
    bad[1, 77, 20:40] = ref[1, 77, 20:40] * 1.01
    fault_report("one pixel of a group with a 1% rstd error", r16(bad), ref, bound, OLD_TOL)


def test_exact_e4m3_codes_and_a_code_off():
    g = torch.Generator().manual_seed(6)
    v = torch.randn(4096, generator=g).double() * 40
    codes = v.clamp(-448, 448).to(torch.float8_e4m3fn).view(torch.uint8)
    assert assert_e4m3_codes(codes, v, 0.0, "exact e4m3") == 0
    # one code off where the value is far from a rounding midpoint: refused
    u = ulp_e4m3(v)
    frac = (v.abs() / u) - (v.abs() / u).floor()
    i = int(((frac - 0.5).abs() - 0.5).abs().argmin())   # nearest to a representable value
    bad = codes.clone()
    bad[i] = bad[i] + 1 if bad[i] & 0x7F < 0x7E else bad[i] - 1
    with pytest.raises(AssertionError):
        assert_e4m3_codes(bad, v, 1e-3 * u, "e4m3 one code off")
    # ... and allowed where the accumulation bound reaches the midpoint
    j = int((frac - 0.5).abs().argmin())
    lo = (v[j].abs() / u[j]).floor() * u[j] * torch.sign(v[j])
    hi = lo + u[j] * torch.sign(v[j])
    pair = torch.stack([lo, hi]).to(torch.float8_e4m3fn).view(torch.uint8)
    alt = codes.clone()
    alt[j] = pair[1] if int(pair[0]) == int(codes[j]) else pair[0]
    assert int(alt[j]) != int(codes[j])
    assert assert_e4m3_codes(alt, v, (frac[j] - 0.5).abs() * u[j] * 1.01, "e4m3 one code at a midpoint") == 1


# ---- the flip budget ---------------------------------------------------------------------------------------------------

FLIP_SHAPES = [(1, 256, 1280), (1, 1024, 1280)]          # gn_small_kernel's largest group (10240 values); the split path


@pytest.fixture(scope="module", params=FLIP_SHAPES, ids=lambda s: "x".join(map(str, s)))
def gn_flip_case(request):
    B, HW, C = request.param
    g = torch.Generator().manual_seed(HW + C)
    x = (torch.randn(B, HW, C, generator=g) * 2 + 0.5).bfloat16().float()
    out = {}
    for kind, silu, scale in (("bf16", True, None), ("e4m3", True, 8.0)):
        if kind == "bf16":
            gamma, beta = torch.randn(C, generator=g), torch.randn(C, generator=g)
        else:
            gamma, beta = torch.randn(C, generator=g) * 0.3 + 1, torch.randn(C, generator=g) * 0.2
        ref, bound = norm_ref_bound(x, gamma, beta, HW * C // 32, 1e-5, silu, groups=32, out_ulp=kind == "bf16")
        if scale:
            ref, bound = ref * scale, bound * scale + U32 * (ref * scale).abs()
        out[kind] = (gamma, beta, silu, scale, ref, bound, gn_restatements(x, gamma, beta, 32, 1e-5, silu, scale))
    return x, out


def old_gate_passes(got32, ref, bound, kind, what):
    if kind == "bf16":
        assert_elementwise(got32.to(torch.bfloat16), ref, bound, what)
    else:
        assert_e4m3_codes(got32.clamp(-448, 448).to(torch.float8_e4m3fn).view(torch.uint8), ref, bound, what)


@pytest.mark.parametrize("kind", ["bf16", "e4m3"])
def test_flip_budget_passes_every_fp32_restatement(gn_flip_case, kind):
    x, cases = gn_flip_case
    _, _, _, _, ref, bound, rest = cases[kind]
    acc = bound - ulp_bf16(ref) if kind == "bf16" else None      # bf16 outputs that cancel to ~0: see assert_flip_budget
    assert len(rest) == 4                                        # two summation orders x two affine forms
    for i, r in enumerate(rest):
        others = rest[:i] + rest[i + 1:]
        got = r.to(torch.bfloat16) if kind == "bf16" else r.clamp(-448, 448).to(torch.float8_e4m3fn).view(torch.uint8)
        flips, f_ref = assert_flip_budget(got, ref, others, kind, f"restatement {i} {kind} {tuple(x.shape)}", acc_bound=acc)
        assert f_ref <= 2.5e-4 * ref.numel()                     # the issue's measurement: 2.3e-4 (bf16), 2e-5 (e4m3) at most
        old_gate_passes(r, ref, bound, kind, f"restatement {i} {kind}, per element")


@pytest.mark.parametrize("kind", ["bf16", "e4m3"])
@pytest.mark.parametrize("mutant", ["eps x 10", "eps x 100", "cnt + 1"])
def test_flip_budget_fails_a_wrong_eps_and_a_wrong_count(gn_flip_case, kind, mutant):
    x, cases = gn_flip_case
    gamma, beta, silu, scale, ref, bound, rest = cases[kind]
    eps, cnt_add = {"eps x 10": (1e-4, 0), "eps x 100": (1e-3, 0), "cnt + 1": (1e-5, 1)}[mutant]
    for form, bad in enumerate(gn_restatements(x, gamma, beta, 32, eps, silu, scale, cnt_add=cnt_add)):
        f_ref = max(count_flips(r, ref, kind) for r in rest)
        flips = count_flips(bad, ref, kind)
        print(f"mutant {mutant} form {form} {kind} {tuple(x.shape)}: flips {flips}, F_ref {f_ref}, numel {ref.numel()}")
        assert flips > 4 * f_ref + 8
        got = bad.to(torch.bfloat16) if kind == "bf16" else bad.clamp(-448, 448).to(torch.float8_e4m3fn).view(torch.uint8)
        with pytest.raises(AssertionError):
            assert_flip_budget(got, ref, rest, kind, f"mutant {mutant} {kind}", acc_bound=bound - ulp_bf16(ref) if kind == "bf16" else None)
        if mutant == "eps x 100":                               # = 1e-3: the gap -- today's per-element gates accept it
            old_gate_passes(bad, ref, bound, kind, f"mutant {mutant} {kind}, per element")


def test_flip_budget_layernorm_restatements_and_helpers():
    g = torch.Generator().manual_seed(11)
    rows, C = 129, 640
    x = (torch.randn(rows, C, generator=g) * 1.5 + 0.2).bfloat16().float()
    gamma, beta = torch.randn(C, generator=g) * 0.3 + 1, torch.randn(C, generator=g) * 0.2
    for kind, scale in (("bf16", None), ("e4m3", 8.0)):
        ref, _ = norm_ref_bound(x, gamma, beta, C, 1e-5, False, out_ulp=False)
        ref = ref * scale if scale else ref
        a, b = ln_restatements(x, gamma, beta, 1e-5, scale)
        got = a.to(torch.bfloat16) if kind == "bf16" else a.clamp(-448, 448).to(torch.float8_e4m3fn).view(torch.uint8)
        assert_flip_budget(got, ref, [b], kind, f"layernorm restatement {kind} {rows}x{C}")
    # the rounding the count is taken against is ONE rounding of the fp64 value; +0 and -0 are the same code
    v = torch.tensor([1.0 + 2.0 ** -8 + 2.0 ** -30, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -0.0, 0.0], dtype=torch.float64)
    assert flip_ordinals(v, "bf16").tolist() == [0x3f81, 0x3f80, 0x3f82, 0, 0]
    e = torch.tensor([17.0, 19.0, 500.0, -500.0, 2.0 ** -10, 3 * 2.0 ** -10, -0.0], dtype=torch.float64)
    assert flip_ordinals(e, "e4m3").tolist() == [0x58, 0x5a, 0x7e, -0x7e, 0, 2, 0]
    assert flip_ordinals(torch.tensor([0x80, 0x00, 0x7e, 0xfe], dtype=torch.uint8), "e4m3").tolist() == [0, 0, 0x7e, -0x7e]
    with pytest.raises(AssertionError):
        flip_ordinals(torch.tensor([0x7f], dtype=torch.uint8), "e4m3")
    # two codes away is refused whatever the budget
    far = torch.tensor([1.0, 2.0], dtype=torch.float64)
    with pytest.raises(AssertionError, match="more than one"):
        assert_flip_budget(torch.tensor([1.0, 2.03125]).bfloat16(), far, [far.float()], "bf16", "two codes off")
    # the interval form of the e4m3 gate: any code between RN(ref - bound) and RN(ref + bound), nothing outside
    r = torch.tensor([-0.00065, 17.3, 100.0], dtype=torch.float64)
    inside = torch.tensor([-0.013671875, 18.0, 104.0]).to(torch.float8_e4m3fn).view(torch.uint8)
    assert assert_e4m3_interval(inside, r, torch.tensor([0.014, 0.5, 1.0], dtype=torch.float64), "interval") == 1
    outside = torch.tensor([-0.017578125, 18.0, 104.0]).to(torch.float8_e4m3fn).view(torch.uint8)
    with pytest.raises(AssertionError):
        assert_e4m3_interval(outside, r, torch.tensor([0.014, 0.5, 1.0], dtype=torch.float64), "interval, one code beyond")
    assert near_midpoint_count(torch.tensor([17.0, 17.1, 18.1, 19.1], dtype=torch.float64), 0.15) == 3   # midpoints 17, 19


# ---- guards -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32, torch.uint8])
@pytest.mark.parametrize("ld", [None, 80])
def test_guards_accept_an_untouched_buffer_and_catch_stray_stores(dtype, ld):
    forget_guards()
    out = guarded((3, 5, 64), dtype, ld=ld, device="cpu", fill=0)
    inp = guarded_input(torch.ones(7, 64), dtype, ld=ld, device="cpu")
    out.fill_(1)                                      # writing the whole tensor itself is fine
    check_guards()
    for where in ("past", "before", "gap"):
        if where == "gap" and ld is None:
            continue
        out = guarded((3, 5, 64), dtype, ld=ld, device="cpu")
        flat = out.as_strided((out.numel() + 2 * 80 * 15,), (1,), out.storage_offset() - 80 * 15)
        end = 80 * 15 + 3 * 5 * (ld or 64)               # one past the last row's pitch
        pos = {"past": end, "before": 80 * 15 - 1, "gap": 80 * 15 + 64}[where]
        flat[pos] = 1
        with pytest.raises(AssertionError, match={"past": "back-guard", "before": "front-guard", "gap": "ld-gap"}[where]):
            check_guards()
    inp = guarded_input(torch.ones(7, 64), dtype, device="cpu")
    if dtype != torch.uint8:
        edge = inp.as_strided((inp.numel() + 2,), (1,), inp.storage_offset() - 1)
        assert torch.isnan(edge[0].float()) and torch.isnan(edge[-1].float())    # reads just outside are poisoned
    check_guards()
