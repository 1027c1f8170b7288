"""GPU parity of every hot kernel, called through the C ABI (sd_op_*), against the stock
PyTorch fp32 CPU operator the reference's CPU path would dispatch to.  Inputs are rounded to
bf16 first so the comparison isolates kernel arithmetic (fp32 accumulate, bf16 output rounding:
tolerance rel-L2 <= 6e-3, i.e. ~1.5 bf16 ulp RMS)."""
import math
import os

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from sonicdiffusionbayeslab_amd import _lib
from tests.bounds import (ATOL_TINY, U32, assert_elementwise, assert_flip_budget, attention_ref_bound, check_guards,
                          conv3x3_nhwc_ref, forget_guards, gemm_bound, gemm_ref, geglu_ref_bound, gn_restatements, guarded,
                          guarded_input, linear_bound, ln_fold_ref_bound, ln_restatements, norm_ref_bound, softmax_rows_ref_bound, subpixel_ref, ulp_bf16,
                          attention_elementwise, conv_gn_elementwise, grouped_softmax_elementwise, ln_fold_elementwise,
                          sample_rows, xattn_elementwise, xattn_norm2_elementwise)

TOL = 6e-3
NHWC = ("b", "y", "x", "c")


def dev(t, dtype=None):
    return t.to("cuda", dtype=dtype) if dtype else t.to("cuda")


def r16(t):
    return t.to(torch.bfloat16).float()


def rel_l2(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return ((a - b).norm() / (b.norm() + 1e-12)).item()


def stream():
    return torch.cuda.current_stream().cuda_stream


_KEEP = []


def P(t, dtype=None):
    """Upload (if needed) and return the device pointer, keeping the tensor alive."""
    if t is None:
        return None
    if t.device.type != "cuda" or (dtype is not None and t.dtype != dtype):
        t = dev(t, dtype)
    _KEEP.append(t)
    return t.data_ptr()


def G(t, dtype=None, **kw):
    """A kernel operand in its own allocation between NaN-poisoned guards (tests/bounds.py)."""
    return guarded_input(t, dtype, **kw)


def OUT(shape, dtype=torch.bfloat16, **kw):
    """A NaN-prefilled kernel output between sentinel guards (tests/bounds.py)."""
    return guarded(shape, dtype, **kw)


def nchw(w, Cout, Cin):
    """[Cout][Cin/64][9][64] packed conv weight -> [Cout, Cin, 3, 3]."""
    return w.float().cpu().view(Cout, Cin // 64, 3, 3, 64).permute(0, 1, 4, 2, 3).reshape(Cout, Cin, 3, 3)






@pytest.fixture(autouse=True)
def _drop_keep():
    yield
    torch.cuda.synchronize()
    _KEEP.clear()
    forget_guards()


@pytest.mark.parametrize("M,N,K,K1,bias,bias2,res", [
    (256, 320, 320, 320, True, False, False),
    (300, 320, 640, 640, True, True, True),
    (130, 640, 960, 640, True, False, True),      # two K segments (virtual concat) + M/N tails
    (64, 1280, 2560, 1280, False, False, False),
    (1000, 960, 320, 320, False, False, False),   # fused QKV shape
])
def test_gemm(sdlib, M, N, K, K1, bias, bias2, res):
    g = torch.Generator().manual_seed(M * 7 + N)
    x = r16(torch.randn(M, K, generator=g))
    w = r16(torch.randn(N, K, generator=g) / math.sqrt(K))
    b = torch.randn(N, generator=g) if bias else None
    b2 = torch.randn(N, generator=g) if bias2 else None
    r = r16(torch.randn(M, N, generator=g)) if res else None
    ref = x @ w.t()
    if bias: ref = ref + b
    if bias2: ref = ref + b2
    if res: ref = ref + r
    x1 = G(x[:, :K1].contiguous(), torch.bfloat16)
    x2 = G(x[:, K1:].contiguous(), torch.bfloat16) if K1 < K else None
    wd = G(w, torch.bfloat16)
    bd = G(b) if bias else None
    b2d = G(b2) if bias2 else None
    rd = G(r, torch.bfloat16) if res else None
    out = OUT((M, N))
    _lib.check(sdlib.sd_op_gemm(stream(), P(x1), K1, P(x2), K - K1, K1, P(wd), P(bd),
                                P(b2d), P(rd), N, P(out), N, M, N, K, 0))
    torch.cuda.synchronize()
    check_guards()
    assert rel_l2(out, ref) < TOL
    assert_elementwise(out, *gemm_bound(x, w, b, b2, r), f"gemm {M}x{N}x{K} K1={K1}", ("row", "col"))


def test_gemm_geglu(sdlib):
    M, C = 200, 320
    g = torch.Generator().manual_seed(3)
    x = r16(torch.randn(M, C, generator=g))
    w = r16(torch.randn(8 * C, C, generator=g) / math.sqrt(C))
    b = torch.randn(8 * C, generator=g)
    proj = x @ w.t() + b
    a, gate = proj.chunk(2, dim=-1)
    ref = a * F.gelu(gate)
    H = 4 * C
    idx = []
    for r in range(2 * H):
        grp, within = divmod(r, 32)
        idx.append(grp * 16 + within if within < 16 else H + grp * 16 + within - 16)
    idx = torch.tensor(idx)
    wp, bp = G(w[idx].contiguous(), torch.bfloat16), G(b[idx].contiguous())
    xd = G(x, torch.bfloat16)
    out = OUT((M, H))
    _lib.check(sdlib.sd_op_gemm(stream(), P(xd), C, None, 0, C, P(wp), P(bp), None, None, 0,
                                P(out), H, M, 8 * C, C, 1))
    torch.cuda.synchronize()
    check_guards()
    assert rel_l2(out, ref) < TOL
    p64, m64 = gemm_ref(x, w, b)
    acc = U32 * (C + 1) * m64
    assert_elementwise(out, *geglu_ref_bound(p64[:, :H], acc[:, :H], p64[:, H:], acc[:, H:]), f"geglu gemm {M}x{H}x{C}",
                       ("row", "col"))


@pytest.mark.parametrize("B,H,Cin,Cout,stride,up,extras", [
    (2, 16, 320, 320, 1, 0, True),
    (1, 16, 640, 320, 1, 0, False),
    (2, 16, 320, 320, 2, 0, False),
    (2, 8, 320, 640, 1, 1, False),
    (3, 6, 64, 64, 1, 0, True),      # M tail (108 rows), single K tile per tap
    (1, 64, 128, 320, 1, 0, True),   # LDS-halo kernel: 4 rows of 64 pixels per tile
    (2, 32, 192, 128, 1, 0, False),  # halo kernel, Cout tail inside the only channel tile
    (3, 16, 320, 192, 1, 0, True),   # halo kernel, one image per tile, partial second channel tile
    (1, 16, 1280, 320, 1, 0, True),  # halo kernel with split-K over channel slices
    (2, 16, 128, 320, 1, 1, True),   # halo kernel, fused upsample to 32x32 (8 output rows per tile)
    (1, 32, 64, 160, 1, 1, False),   # halo kernel, fused upsample to 64x64
    (5, 8, 256, 192, 1, 0, True),    # halo kernel, 4 whole 8x8 images per tile + an M tail tile
    (1, 4, 64, 64, 1, 1, False),     # upsample to 8x8: one image, 192 of 256 tile rows unused
])
def test_conv3x3(sdlib, B, H, Cin, Cout, stride, up, extras):
    g = torch.Generator().manual_seed(B * 100 + H + Cin)
    x = r16(torch.randn(B, Cin, H, H, generator=g))
    w = r16(torch.randn(Cout, Cin, 3, 3, generator=g) / math.sqrt(9 * Cin))
    b = torch.randn(Cout, generator=g)
    xin = F.interpolate(x, scale_factor=2.0, mode="nearest") if up else x
    ref = F.conv2d(xin, w, b, stride=stride, padding=1)
    Ho = ref.shape[-1]
    b2 = r = None
    if extras:
        b2 = torch.randn(Cout, generator=g)
        r = r16(torch.randn(B, Cout, Ho, Ho, generator=g))
        ref = ref + b2[None, :, None, None] + r
    xd = G(x.permute(0, 2, 3, 1).contiguous(), torch.bfloat16)
    wd = G(w.permute(0, 2, 3, 1).reshape(Cout, 9, Cin // 64, 64).permute(0, 2, 1, 3).contiguous(), torch.bfloat16)
    rd = G(r.permute(0, 2, 3, 1).contiguous(), torch.bfloat16) if extras else None
    out = OUT((B, Ho, Ho, Cout))
    _lib.check(sdlib.sd_op_conv3x3(stream(), P(xd), P(wd), P(G(b)),
                                   P(G(b2)) if extras else None, P(rd), P(out), B, H, H, Cin,
                                   Cout, stride, up))
    torch.cuda.synchronize()
    check_guards()
    assert rel_l2(out.permute(0, 3, 1, 2), ref) < TOL
    r64, m64 = conv3x3_nhwc_ref(x, w, b, b2, r, stride, up)
    assert_elementwise(out, r64, linear_bound(r64, m64, 9 * Cin + 3), f"conv3x3 B={B} H={H} {Cin}->{Cout} s{stride} up{up}", NHWC)


@pytest.mark.parametrize("B,H,Cin,Cout", [(2, 64, 128, 320), (3, 16, 320, 192), (5, 8, 256, 192), (1, 32, 640, 640)])
def test_conv3x3_halo_four_wave_layout_is_bit_identical(sdlib, B, H, Cin, Cout):
    """The A/B layout of the halo kernel (4 waves of 128 x 80 outputs, the second k-step of a tap carried over the next tap's
    barrier; sd_op_conv3x3_ablate mode 256 of the SD_ABLATE build, libsdhip_ablate.so) issues every accumulator's MFMAs in
    the product kernel's order: the same bits as the PRODUCT library's kernel.  The product library itself refuses every
    ablation mode: it carries none of those kernels."""
    abl = _lib.load_ablate()
    g = torch.Generator().manual_seed(B + H + Cin)
    xd = G(r16(torch.randn(B, H, H, Cin, generator=g)), torch.bfloat16)
    wd = G(r16(torch.randn(Cout, Cin // 64, 9, 64, generator=g) / math.sqrt(9 * Cin)), torch.bfloat16)
    outs = []
    for lib, mode in ((sdlib, 0), (abl, 0), (abl, 256)):
        out = OUT((B, H, H, Cout))
        _lib.check(lib.sd_op_conv3x3_ablate(stream(), P(xd), P(wd), P(out), B, H, H, Cin, Cout, mode), lib=lib)
        torch.cuda.synchronize()
        outs.append(out)
    check_guards()
    r64, m64 = conv3x3_nhwc_ref(xd.float().cpu().permute(0, 3, 1, 2), nchw(wd, Cout, Cin))
    assert_elementwise(outs[0], r64, linear_bound(r64, m64, 9 * Cin), f"conv3x3 halo B={B} H={H} {Cin}->{Cout}", NHWC)
    assert torch.isfinite(outs[0].float()).all()
    assert torch.equal(outs[0].view(torch.int16), outs[1].view(torch.int16))
    assert torch.equal(outs[0].view(torch.int16), outs[2].view(torch.int16))
    for mode in (8, 256):
        assert sdlib.sd_op_conv3x3_ablate(stream(), P(xd), P(wd), P(outs[1]), B, H, H, Cin, Cout, mode) != 0


def _subpixel_weights(w):
    """[Cout, Cin, 3, 3] -> [4 phases][Cout][Cin/64][4 taps][64]: the 3x3 taps that read the same low-res pixel, summed."""
    Cout, Cin = w.shape[:2]
    rows = {0: ([0], [1, 2]), 1: ([0, 1], [2])}                       # phase -> 3x3 taps behind 2x2 tap 0 / 1
    w4 = torch.zeros(4, Cout, Cin, 2, 2)
    for py in (0, 1):
        for px in (0, 1):
            for dy in (0, 1):
                for dx in (0, 1):
                    w4[py * 2 + px, :, :, dy, dx] = w[:, :, rows[py][dy]][:, :, :, rows[px][dx]].sum((2, 3))
    return w4.permute(0, 1, 3, 4, 2).reshape(4, Cout, 4, Cin // 64, 64).permute(0, 1, 3, 2, 4).contiguous()


@pytest.mark.parametrize("B,H,Cin,Cout", [(2, 16, 128, 320), (1, 32, 64, 192), (3, 16, 320, 100), (5, 8, 128, 320),
                                          (16, 16, 128, 1280),     # >= 256 work items: the halo kernel's 4-tap mode
                                          (4, 32, 192, 640),       # ... four 256-pixel tiles per image
                                          (32, 16, 64, 200),       # ... Cout tail in the second channel tile
                                          (48, 8, 128, 1280)])     # 8x8 input with UNet batch >= 32 (batch 16 + CFG): the 4-tap mode's
                                                                   # multi-image tiles (4 images per 256-pixel tile; 12 x 4 x 8 = 384 items)
def test_conv3x3_upsample_as_four_subpixel_convs(sdlib, B, H, Cin, Cout):
    """Upsample2D = nearest 2x + 3x3 conv, computed as four 2x2 convs on the low-res input (one per output phase) with
    summed taps: the same linear map with 4/9 of the multiply-adds; against interpolate + conv2d.  Large grids run on the
    halo kernel's 4-tap mode (csrc/conv_halo.hip, SUB): same K order and accumulation chains as the implicit-GEMM kernel,
    so the two agree bit for bit (SD_SUBPIX_HALO=0 selects the latter)."""
    g = torch.Generator().manual_seed(H + Cin + Cout)
    x = r16(torch.randn(B, Cin, H, H, generator=g))
    w = r16(torch.randn(Cout, Cin, 3, 3, generator=g) / math.sqrt(9 * Cin))
    b = torch.randn(Cout, generator=g)
    ref = F.conv2d(F.interpolate(x, scale_factor=2.0, mode="nearest"), w, b, padding=1)
    w4p = _subpixel_weights(w)
    xd = G(x.permute(0, 2, 3, 1).contiguous(), torch.bfloat16)
    w4d, bd = G(w4p, torch.bfloat16), G(b)

    def run():
        out = OUT((B, 2 * H, 2 * H, Cout))
        _lib.check(sdlib.sd_op_conv3x3_upsample_subpixel(stream(), P(xd), P(w4d), P(bd), P(out), B, H, H, Cin, Cout))
        torch.cuda.synchronize()
        return out
    out = run()
    assert rel_l2(out.permute(0, 3, 1, 2), ref) < TOL
    # elementwise: from the bf16-rounded summed phase weights the kernel reads (their rounding is the formulation's)
    r64, m64 = subpixel_ref(x, w4p.to(torch.bfloat16), b)
    assert_elementwise(out, r64, linear_bound(r64, m64, 4 * Cin + 1), f"conv3x3 subpixel B={B} H={H} {Cin}->{Cout}", NHWC)
    os.environ["SD_SUBPIX_HALO"] = "0"
    try:
        other = run()
    finally:
        del os.environ["SD_SUBPIX_HALO"]
    check_guards()
    assert torch.equal(out.view(torch.int16), other.view(torch.int16))


@pytest.mark.parametrize("B,H,Cin,Cout", [(16, 16, 128, 640),      # halo kernel's 4-tap mode, one tile per image
                                          (4, 32, 64, 640),        # ... four tiles per image
                                          (2, 16, 128, 320)])      # implicit-GEMM kernel
                                                                   # (8x8 inputs carry no producer statistics: 64-pixel phases)
def test_conv3x3_upsample_subpixel_groupnorm_producer_statistics(sdlib, B, H, Cin, Cout):
    """Upsample2D -> the next resnet's GroupNorm with the statistics from the conv epilogue: 64-row blocks in the row order
    (sample, phase, low-res pixel), whichever kernel ran the conv.  The "own statistics" leg also gets the flip budget;
    measured flips / F_ref / numel: 363 / 1325 / 10485760, 340 / 2326 / 10485760, 33 / 102 / 655360."""
    g = torch.Generator().manual_seed(H + Cin + Cout + 1)
    x = r16(torch.randn(B, Cin, H, H, generator=g))
    w = r16(torch.randn(Cout, Cin, 3, 3, generator=g) / math.sqrt(9 * Cin))
    b = torch.randn(Cout, generator=g)
    gamma, beta = torch.randn(Cout, generator=g), torch.randn(Cout, generator=g)
    conv = r16(F.conv2d(F.interpolate(x, scale_factor=2.0, mode="nearest"), w, b, padding=1))
    ref = F.silu(F.group_norm(conv, 32, gamma, beta, 1e-5))
    xd = G(x.permute(0, 2, 3, 1).contiguous(), torch.bfloat16)
    w4p = _subpixel_weights(w)
    gd, btd = G(gamma), G(beta)
    y = OUT((B, 2 * H, 2 * H, Cout))
    yn = OUT((B, 2 * H, 2 * H, Cout))
    _lib.check(sdlib.sd_op_conv3x3_upsample_subpixel_groupnorm(stream(), P(xd), P(G(w4p, torch.bfloat16)), P(G(b)), P(y),
                                                               B, H, H, Cin, Cout, P(gd), P(btd), P(yn), 32, 1e-5, 1))
    torch.cuda.synchronize()
    assert rel_l2(y.permute(0, 3, 1, 2), conv) < TOL
    assert rel_l2(yn.permute(0, 3, 1, 2), ref) < TOL
    own = OUT((B, 2 * H, 2 * H, Cout))
    _lib.check(sdlib.sd_op_groupnorm(stream(), P(y), Cout, None, 0, P(gd), P(btd), P(own), B, 4 * H * H, 32, 1e-5, 1))
    torch.cuda.synchronize()
    check_guards()
    assert rel_l2(yn, own) < 2e-3
    r64, m64 = subpixel_ref(x, w4p.to(torch.bfloat16), b)
    assert_elementwise(y, r64, linear_bound(r64, m64, 4 * Cin + 1), f"conv3x3 subpixel+gn conv B={B} H={H} {Cin}->{Cout}", NHWC)
    # the normalisation, chained from the kernel's own stored conv output
    yk = y.float().cpu().view(B, 4 * H * H, Cout)
    n64, nb = norm_ref_bound(yk, gamma, beta, 4 * H * H * Cout // 32, 1e-5, True, groups=32)
    for t, name in ((yn, "producer statistics"), (own, "own statistics")):
        assert_elementwise(t.view(B, 4 * H * H, Cout), n64, nb, f"groupnorm after subpixel conv ({name}) B={B} H={H} C={Cout}",
                           ("b", "pixel", "c"))
    assert_flip_budget(own.view(B, 4 * H * H, Cout), n64, gn_restatements(yk, gamma, beta, 32, 1e-5, True), "bf16",
                       f"groupnorm after subpixel conv (own statistics) B={B} H={H} C={Cout}", acc_bound=nb - ulp_bf16(n64))


@pytest.mark.parametrize("B,HW,C1,C2,silu,eps", [
    (2, 256, 320, 0, 1, 1e-5),
    (2, 64, 640, 320, 1, 1e-5),     # concat 960: groups of 30 straddle the tensor boundary
    (1, 1024, 1280, 1280, 0, 1e-6),
    (3, 16, 1280, 640, 1, 1e-5),    # single-launch small-image kernel, a group straddles the concat boundary
    (2, 64, 1280, 1280, 1, 1e-5),   # small-image kernel at the 8x8 level (80 channels per group)
    (5, 64, 1280, 0, 0, 1e-6),      # ... 40 channels per group, no SiLU
    # the VAE's channel counts (128 / 256 / 512 = 4 / 8 / 16 channels per group, eps 1e-6)
    (1, 4096, 128, 0, 1, 1e-6),     # split path, 4 channels per group: every 8-channel chunk straddles two groups
    (2, 1000, 128, 0, 0, 1e-6),     # ... with a ragged pixel split
    (2, 64, 128, 0, 1, 1e-6),       # gn_small_kernel with one 4-channel unit per pixel
    (1, 1024, 256, 0, 1, 1e-6),     # 8 channels per group
    (2, 256, 512, 0, 1, 1e-6),      # gn_small_kernel, 16 channels per group: the VAE mid block at a 16x16 latent
    (1, 4096, 512, 0, 0, 1e-6),     # split path, 16 channels per group: the attention's GroupNorm
])
def test_groupnorm(sdlib, B, HW, C1, C2, silu, eps):
    """Against torch, per element (norm_ref_bound), and by count (assert_flip_budget: outputs that are not the correctly
    rounded fp64 value, against four fp32 restatements of the kernels' formulas on the CPU, budget 4 F_ref + 8).
    Measured, flips / F_ref / numel in the order of the cases: 2 / 9 / 163840, 1 / 3 / 122880, 97 / 392 / 2621440,
    2 / 3 / 92160, 17 / 21 / 327680, 15 / 31 / 409600; the VAE's widths: 12 / 125 / 524288, 10 / 51 / 256000, 0 / 0 / 16384,
    11 / 30 / 262144, 9 / 12 / 262144, 74 / 493 / 2097152.  No kernel needed an addition to its restatement."""
    g = torch.Generator().manual_seed(HW + C1)
    C = C1 + C2
    x = r16(torch.randn(B, HW, C, generator=g) * 2 + 0.5)
    gamma, beta = torch.randn(C, generator=g), torch.randn(C, generator=g)
    ref = F.group_norm(x.permute(0, 2, 1), 32, gamma, beta, eps)
    if silu: ref = F.silu(ref)
    ref = ref.permute(0, 2, 1)
    x1 = G(x[..., :C1].contiguous(), torch.bfloat16)
    x2 = G(x[..., C1:].contiguous(), torch.bfloat16) if C2 else None
    out = OUT((B, HW, C))
    _lib.check(sdlib.sd_op_groupnorm(stream(), P(x1), C1, P(x2), C2, P(G(gamma)),
                                     P(G(beta)), P(out), B, HW, 32, eps, silu))
    torch.cuda.synchronize()
    check_guards()
    assert rel_l2(out, ref) < TOL
    n64, nb = norm_ref_bound(x, gamma, beta, HW * C // 32, eps, silu, groups=32)
    assert_elementwise(out, n64, nb, f"groupnorm B={B} HW={HW} C={C1}+{C2}", ("b", "pixel", "c"))
    assert_flip_budget(out, n64, gn_restatements(x, gamma, beta, 32, eps, silu), "bf16", f"groupnorm B={B} HW={HW} C={C1}+{C2}",
                       acc_bound=nb - ulp_bf16(n64))


@pytest.mark.parametrize("B,H,Cin,Cout", [
    (2, 64, 128, 320),     # LDS-halo conv, two channel tiles
    (3, 32, 192, 640),     # halo conv, 16 blocks of 64 pixels per sample
    (1, 32, 320, 1280),    # 40 channels per group (16x16 and below run the single-launch GroupNorm: no statistics)
    (1, 32, 64, 256),      # 8 channels per group, Cout tail in the second channel tile
])
def test_conv3x3_groupnorm_producer_statistics(sdlib, B, H, Cin, Cout):
    """The plan's conv -> GroupNorm pair: statistics come from the conv epilogue (sums of the bf16-rounded outputs).
    The "own statistics" leg also gets the flip budget; measured flips / F_ref / numel: 128 / 733 / 2621440, 63 / 251 / 1966080,
    43 / 97 / 1310720, 0 / 22 / 262144."""
    g = torch.Generator().manual_seed(H + Cin + Cout)
    x = r16(torch.randn(B, Cin, H, H, generator=g))
    w = r16(torch.randn(Cout, Cin, 3, 3, generator=g) / math.sqrt(9 * Cin))
    b, b2 = torch.randn(Cout, generator=g), torch.randn(Cout, generator=g)
    r = r16(torch.randn(B, Cout, H, H, generator=g))
    gamma, beta = torch.randn(Cout, generator=g), torch.randn(Cout, generator=g)
    conv = r16(F.conv2d(x, w, b, padding=1) + b2[None, :, None, None] + r)
    ref = F.silu(F.group_norm(conv, 32, gamma, beta, 1e-5))
    xd = G(x.permute(0, 2, 3, 1).contiguous(), torch.bfloat16)
    wd = G(w.permute(0, 2, 3, 1).reshape(Cout, 9, Cin // 64, 64).permute(0, 2, 1, 3).contiguous(), torch.bfloat16)
    rd = G(r.permute(0, 2, 3, 1).contiguous(), torch.bfloat16)
    gd, btd = G(gamma), G(beta)
    y = OUT((B, H, H, Cout))
    yn = OUT((B, H, H, Cout))
    _lib.check(sdlib.sd_op_conv3x3_groupnorm(stream(), P(xd), P(wd), P(G(b)), P(G(b2)), P(rd), P(y), B, H, H, Cin, Cout,
                                             P(gd), P(btd), P(yn), 32, 1e-5, 1))
    torch.cuda.synchronize()
    assert rel_l2(y.permute(0, 3, 1, 2), conv) < TOL
    assert rel_l2(yn.permute(0, 3, 1, 2), ref) < TOL
    # and the same GroupNorm computing its own statistics from the stored tensor agrees to rounding
    own = OUT((B, H, H, Cout))
    _lib.check(sdlib.sd_op_groupnorm(stream(), P(y), Cout, None, 0, P(gd), P(btd), P(own), B, H * H, 32, 1e-5, 1))
    torch.cuda.synchronize()
    check_guards()
    assert rel_l2(yn, own) < 2e-3
    conv_gn_elementwise(x, w, b, b2, r, gamma, beta, y, (yn, own), f"conv3x3+gn B={B} H={H} {Cin}->{Cout}", flip=(1,))




@pytest.mark.parametrize("B,H,Cin,Cout,res", [
    (16, 8, 512, 1280, True),      # 8x8: 32 output tiles, split-K 8 on the halo kernel; 3 units per thread, 8 slabs per trip
    (16, 16, 512, 1280, True),     # 16x16: split-K 2; 10 units per thread, 2 slabs per trip
    (8, 8, 512, 2560, False),      # 80 channels per group (5 units per thread), split-K 4, no residual
    (6, 16, 384, 640, True),       # 20 channels per group, split-K 3 (odd: one slab per trip)
    (3, 4, 256, 1280, True),       # 4x4 images: the implicit-GEMM conv kernel's split-K
])
def test_conv3x3_groupnorm_small_images_finish_the_deferred_splitk_reduce(sdlib, B, H, Cin, Cout, res):
    """The plan's conv -> GroupNorm pair at the 8x8 / 16x16 levels (diffusers ResnetBlock2D: conv1 -> norm2, conv2 -> the next
    block's norm1): a split-K conv leaves its fp32 partial slabs to the single-launch GroupNorm, which sums them in
    splitk_reduce_kernel's order, adds bias / time-embedding row / residual, stores the conv output and normalises it -- one
    launch instead of two.  Bit-identical to conv (+ reduce) followed by the GroupNorm (SD_GN_SLAB=0), and right."""
    g = torch.Generator().manual_seed(H + Cin + Cout)
    x = r16(torch.randn(B, Cin, H, H, generator=g))
    w = r16(torch.randn(Cout, Cin, 3, 3, generator=g) / math.sqrt(9 * Cin))
    b, b2 = torch.randn(Cout, generator=g), torch.randn(Cout, generator=g)
    r = r16(torch.randn(B, Cout, H, H, generator=g)) if res else None
    gamma, beta = torch.randn(Cout, generator=g), torch.randn(Cout, generator=g)
    conv = r16(F.conv2d(x, w, b, padding=1) + b2[None, :, None, None] + (r if res else 0.0))
    ref = F.silu(F.group_norm(conv, 32, gamma, beta, 1e-5))
    xd = G(x.permute(0, 2, 3, 1).contiguous(), torch.bfloat16)
    wd = G(w.permute(0, 2, 3, 1).reshape(Cout, 9, Cin // 64, 64).permute(0, 2, 1, 3).contiguous(), torch.bfloat16)
    rd = G(r.permute(0, 2, 3, 1).contiguous(), torch.bfloat16) if res else None
    bd, b2d, gd, btd = G(b), G(b2), G(gamma), G(beta)

    def run():
        y = OUT((B, H, H, Cout))
        yn = OUT((B, H, H, Cout))
        _lib.check(sdlib.sd_op_conv3x3_groupnorm(stream(), P(xd), P(wd), P(bd), P(b2d), P(rd) if res else None, P(y), B, H, H, Cin,
                                                 Cout, P(gd), P(btd), P(yn), 32, 1e-5, 1))
        torch.cuda.synchronize()
        return y, yn
    assert sdlib.sd_op_conv3x3_splitk(B * H * H, Cout, Cin, H, H, 1, 0) > 1       # the case exists to exercise the slabs
    y, yn = run()
    assert rel_l2(y.permute(0, 3, 1, 2), conv) < TOL
    assert rel_l2(yn.permute(0, 3, 1, 2), ref) < TOL
    os.environ["SD_GN_SLAB"] = "0"
    try:
        y2, yn2 = run()
    finally:
        del os.environ["SD_GN_SLAB"]
    check_guards()
    assert torch.equal(y.view(torch.int16), y2.view(torch.int16))
    assert torch.equal(yn.view(torch.int16), yn2.view(torch.int16))
    conv_gn_elementwise(x, w, b, b2, r, gamma, beta, y, (yn,), f"conv3x3+gn split-K B={B} H={H} {Cin}->{Cout}")


def fold_layernorm(w, gamma, beta, bias):
    """Host-side packing of a LayerNorm-folded GEMM weight (mirror of the packer's ln_fold in pack.hip)."""
    wg = r16(w * gamma[None, :])
    c1 = wg.double().sum(1).float()
    c2 = (w.double() @ beta.double()).float() + (bias if bias is not None else 0.0)
    return wg, c1, c2


@pytest.mark.parametrize("M,C,N2,epi,mean", [
    (256, 320, 960, 0, 0.0),       # norm1 -> q|k|v at the 64x64 level's width
    (192, 640, 5120, 1, 0.5),      # norm3 -> GEGLU (256 x 256 tile), rows with a common offset
    (128, 1280, 3840, 0, 2.0),     # 16 partials per row, |mean| ~ sigma
    (320, 320, 2560, 1, 0.0),      # GEGLU, M tail in the 256-row tile
    (200, 320, 960, 0, 0.0),       # M tail (rows 192..199 of the last 64-row block)
])
def test_layernorm_folded_into_gemm(sdlib, M, C, N2, epi, mean):
    """h = X W1^T + b1 + R with per-row partials from the epilogue, then Y = epi(LN(h) W2^T + b2) computed by the GEMM on the
    un-normalised h (diffusers BasicTransformerBlock norm1 -> attn1 / norm3 -> ff): against LayerNorm + linear in fp32."""
    g = torch.Generator().manual_seed(M + C + N2)
    x = r16(torch.randn(M, C, generator=g))
    w1 = r16(torch.randn(C, C, generator=g) / math.sqrt(C))
    b1 = torch.randn(C, generator=g) + mean
    r = r16(torch.randn(M, C, generator=g) * 2)
    r[:, 7] += 12.0                                   # an outlier channel, as the SD residual stream has
    gamma, beta = torch.randn(C, generator=g), torch.randn(C, generator=g)
    w2 = torch.randn(N2, C, generator=g) / math.sqrt(C)
    b2 = torch.randn(N2, generator=g)
    h = r16(x @ w1.t() + b1 + r)
    z = F.layer_norm(h, (C,), gamma, beta, 1e-5) @ r16(w2).t() + b2
    if epi:
        H = N2 // 2
        ref = z[:, :H] * F.gelu(z[:, H:])
        idx = torch.tensor([(q // 32) * 16 + q % 32 if q % 32 < 16 else H + (q // 32) * 16 + q % 32 - 16 for q in range(N2)])
        w2p, b2p = w2[idx], b2[idx]
    else:
        ref, w2p, b2p = z, w2, b2
    wg, c1, c2 = fold_layernorm(w2p, gamma, beta, b2p)
    parts = sdlib.sd_op_ln_partials(0, M, C)
    assert parts == 2 * ((C + 159) // 160)
    hd = OUT((M, C))
    rs = OUT((parts, M, 2), torch.float32)
    _lib.check(sdlib.sd_op_gemm_rowstats(stream(), P(G(x, torch.bfloat16)), C, P(G(w1, torch.bfloat16)), P(G(b1)),
                                         P(G(r, torch.bfloat16)), C, P(hd), C, M, C, C, P(rs)))
    torch.cuda.synchronize()
    assert rel_l2(hd, h) < TOL
    assert_elementwise(hd, *gemm_bound(x, w1, b1, None, r16(r)), f"gemm rowstats {M}x{C}", ("row", "col"))
    tot, h64 = rs.sum(0).cpu().double(), hd.double().cpu()
    assert torch.allclose(tot[:, 0], h64.sum(1), rtol=1e-4, atol=1e-2)
    assert torch.allclose(tot[:, 1], (h64 * h64).sum(1), rtol=1e-4, atol=1e-2)
    # partials: fp32 sums of the stored bf16 values (C / parts terms each, then the partials' own sum here)
    sl = h64.view(M, parts, C // parts).permute(1, 0, 2)
    for j, (want, mag) in enumerate(((sl.sum(-1), sl.abs().sum(-1)), ((sl * sl).sum(-1), (sl * sl).sum(-1)))):
        assert_elementwise(rs[..., j], want, U32 * (C // parts + 1) * mag + ATOL_TINY, f"gemm rowstats partial[{j}] {M}x{C}",
                           ("part", "row"))
    No = N2 // 2 if epi else N2
    out = OUT((M, No))
    _lib.check(sdlib.sd_op_gemm_ln(stream(), P(hd), C, P(G(wg, torch.bfloat16)), P(G(c1)), P(G(c2)), P(rs), parts, 1e-5,
                                   P(out), No, M, N2, C, epi))
    torch.cuda.synchronize()
    check_guards()
    ln_fold_elementwise(out, hd, wg, c1, c2, rs, epi, f"gemm_ln {M}x{N2}x{C} epi{epi}", idx=idx if epi else None)
    # reference from the device's own h (the fold is judged, not the producer's rounding)
    hh = hd.float().cpu()
    z = F.layer_norm(hh, (C,), gamma, beta, 1e-5) @ r16(w2).t() + b2
    ref = z[:, :N2 // 2] * F.gelu(z[:, N2 // 2:]) if epi else z
    assert rel_l2(out, ref) < TOL




def _gemm_plan(sdlib, lean, x, x2, w, b, b2, r, M, N, K, K1, want_rs=False, want_st=False, ln=None, hm_tokens=0):
    """One sd_op_gemm_plan call on the lean (gemm_lean.hip) or the general (gemm_conv.hip) kernel.  Returns (C, rowstats,
    stats, KV) -- untouched outputs stay NaN."""
    import os
    os.environ["SD_GEMM_LEAN"] = "1" if lean else "0"
    try:
        ncols = N // 3 if hm_tokens else N
        out = OUT((M, ncols))
        rs = OUT((2 * (N // 160), M, 2), torch.float32) if want_rs else None
        st = OUT((M // 64, N, 2), torch.float32) if want_st else None
        kv = OUT((2, M // hm_tokens, ncols // 40, hm_tokens, 40)) if hm_tokens else None
        ln_rs, ln_parts, ln_c1 = ln if ln else (None, 0, None)
        _lib.check(sdlib.sd_op_gemm_plan(stream(), P(x), K1, P(x2), K - K1, K1, P(w), P(b), P(b2), P(r), N, P(out), ncols, M, N, K,
                                         P(rs), P(st), P(ln_rs), ln_parts, P(ln_c1), 1e-5, P(kv), hm_tokens))
        torch.cuda.synchronize()
        return out, rs, st, kv
    finally:
        os.environ.pop("SD_GEMM_LEAN", None)


@pytest.mark.parametrize("M,N,K,K1,bias,bias2,res,rowstats,stats", [
    (256, 320, 320, 320, True, False, False, False, False),
    (384, 640, 1600, 1280, True, False, True, False, True),      # merged ff.net.2 + proj_out: two K segments, residual, block statistics
    (256, 320, 320, 320, True, False, True, True, False),        # to_out / proj_in: residual + LayerNorm row partials
    (130, 960, 640, 640, False, False, False, False, False),     # M tail: rows beyond M read zeros, their stores are dropped
    (64, 1280, 2560, 1280, True, True, True, False, False),      # 64-row tiles never mix samples; bias2
    (1000, 160, 128, 128, True, True, False, False, False),      # smallest K the lean kernel takes (two K tiles), one N tile
])
def test_gemm_lean_kernel_is_bit_identical_to_the_general_kernel(sdlib, M, N, K, K1, bias, bias2, res, rowstats, stats):
    """csrc/gemm_lean.hip re-builds the std-epilogue GEMM of the UNet's projections around buffer addressing (a fraction of
    the per-item instructions); same tile, same accumulation order, same rounding points -> the same BITS as gemm_kernel,
    for every side input / output the plan combines (call site src/models.py:227-235).  Also vs fp32 torch."""
    g = torch.Generator().manual_seed(M + N + K)
    x = r16(torch.randn(M, K, generator=g))
    w = r16(torch.randn(N, K, generator=g) / math.sqrt(K))
    b = torch.randn(N, generator=g) if bias else None
    b2 = torch.randn(N, generator=g) if bias2 else None
    r = r16(torch.randn(M, N, generator=g)) if res else None
    x1 = G(x[:, :K1].contiguous(), torch.bfloat16)
    x2 = G(x[:, K1:].contiguous(), torch.bfloat16) if K1 < K else None
    args = (x1, x2, G(w, torch.bfloat16), G(b) if bias else None, G(b2) if bias2 else None,
            G(r, torch.bfloat16) if res else None, M, N, K, K1, rowstats, stats)
    lean, general = _gemm_plan(sdlib, True, *args), _gemm_plan(sdlib, False, *args)
    check_guards()
    assert_elementwise(lean[0], *gemm_bound(x, w, b, b2, r), f"gemm lean {M}x{N}x{K} K1={K1}", ("row", "col"))
    ref = x @ w.t()
    for t in (b, b2, r):
        if t is not None:
            ref = ref + t
    assert rel_l2(lean[0], ref) < TOL
    for a, c in zip(lean, general):
        assert (a is None) == (c is None)
        if a is not None:
            assert torch.isfinite(a.float()).all() and torch.equal(a, c)


@pytest.mark.parametrize("B,tokens,C,mean", [(2, 4096, 320, 0.0), (1, 256, 640, 1.5), (1, 128, 1280, 0.3)])
def test_gemm_lean_layernorm_fold_and_headmajor_kv(sdlib, B, tokens, C, mean):
    """The q|k|v projection as the plan runs it at the 64x64 level: LayerNorm folded in (4 / 8 / 16 row partials) AND K / V
    stored head-major, on the lean kernel -- bit-identical to the general kernel, and its head-major K / V are exactly the
    token-major columns of the same call without the head-major option, re-ordered."""
    M, N = B * tokens, 3 * C
    g = torch.Generator().manual_seed(B + tokens + C)
    h = r16(torch.randn(M, C, generator=g) * 2 + mean)
    h[:, 3] += 9.0                                   # an outlier channel
    gamma, beta = torch.randn(C, generator=g), torch.randn(C, generator=g)
    w = torch.randn(N, C, generator=g) / math.sqrt(C)
    wg, c1, c2 = fold_layernorm(w, gamma, beta, torch.zeros(N))
    parts = 2 * (C // 160)
    hh = h.view(M, parts, C // parts)
    rs = torch.stack([hh.sum(2), (hh * hh).sum(2)], dim=2).permute(1, 0, 2).contiguous()      # [parts][M][2]
    ln = (G(rs), parts, G(c1))
    args = (G(h, torch.bfloat16), None, G(wg, torch.bfloat16), G(c2), None, None, M, N, C, C)
    plain = _gemm_plan(sdlib, True, *args, ln=ln)[0]
    ref = F.layer_norm(h, (C,), gamma, beta, 1e-5) @ r16(w).t()
    assert rel_l2(plain, ref) < TOL
    ln_fold_elementwise(plain, h, wg, c1, c2, rs, 0, f"gemm lean ln-fold {M}x{N}x{C}")
    assert torch.equal(plain, _gemm_plan(sdlib, False, *args, ln=ln)[0])
    if C // 40 == 8:                                 # head dim 40, >= 8192 rows (128-row tiles): the 64x64 level's layout
        for lean in (True, False):
            q, _, _, kv = _gemm_plan(sdlib, lean, *args, ln=ln, hm_tokens=tokens)
            assert torch.equal(q, plain[:, :C])
            for which in (0, 1):
                want = plain[:, (1 + which) * C:(2 + which) * C].reshape(B, tokens, C // 40, 40).permute(0, 2, 1, 3)
                assert torch.equal(kv[which], want)
    check_guards()


@pytest.mark.parametrize("M,C,fold", [(512, 320, True), (256, 640, True), (256, 1280, True), (512, 320, False), (300, 640, False),
                                      (512, 320, 2)])      # 2 partials per row: the fused cross-attention's at the 64x64 level
def test_gemm_lean_geglu_kernel_is_bit_identical_to_the_general_kernel(sdlib, M, C, fold):
    """The GEGLU projection (ff.net.0.proj, N = 8 C packed [16 value | 16 gate]) on the lean 256 x 256 kernel of
    csrc/gemm_lean.hip -- with the LayerNorm fold (4 / 8 / 16 row partials: norm3 -> GEGLU as the plan runs it) and with a
    plain bias (incl. an M tail) -- against fp32 torch and, bit for bit, against gemm_kernel's GEGLU instantiation."""
    import os
    g = torch.Generator().manual_seed(M + C)
    N, H = 8 * C, 4 * C
    h = r16(torch.randn(M, C, generator=g) * 1.5 + 0.4)
    w = torch.randn(N, C, generator=g) / math.sqrt(C)
    b = torch.randn(N, generator=g)
    idx = torch.tensor([(q // 32) * 16 + q % 32 if q % 32 < 16 else H + (q // 32) * 16 + q % 32 - 16 for q in range(N)])
    outs = []
    if fold:
        gamma, beta = torch.randn(C, generator=g), torch.randn(C, generator=g)
        z = F.layer_norm(h, (C,), gamma, beta, 1e-5) @ r16(w).t() + b
        wg, c1, c2 = fold_layernorm(w[idx], gamma, beta, b[idx])
        parts = 2 * (C // 160) if fold is True else int(fold)
        hh = h.view(M, parts, C // parts)
        rs = G(torch.stack([hh.sum(2), (hh * hh).sum(2)], dim=2).permute(1, 0, 2).contiguous())
        hd, wd, c1d, c2d = G(h, torch.bfloat16), G(wg, torch.bfloat16), G(c1), G(c2)
    else:
        z = h @ r16(w).t() + b
        hd, wd, bd = G(h, torch.bfloat16), G(w[idx].contiguous(), torch.bfloat16), G(b[idx].contiguous())
    ref = z[:, :H] * F.gelu(z[:, H:])
    for lean in ("1", "0"):
        os.environ["SD_GEMM_LEAN"] = lean
        try:
            out = OUT((M, H))
            if fold:
                _lib.check(sdlib.sd_op_gemm_ln(stream(), P(hd), C, P(wd), P(c1d), P(c2d), P(rs), parts, 1e-5, P(out), H, M, N, C, 1))
            else:
                _lib.check(sdlib.sd_op_gemm(stream(), P(hd), C, None, 0, C, P(wd), P(bd), None, None, 0, P(out), H, M, N, C, 1))
            torch.cuda.synchronize()
        finally:
            os.environ.pop("SD_GEMM_LEAN", None)
        outs.append(out)
    assert torch.isfinite(outs[0].float()).all() and rel_l2(outs[0], ref) < TOL
    assert torch.equal(outs[0], outs[1])
    check_guards()
    if fold:
        ln_fold_elementwise(outs[0], h, wg, c1, c2, rs, 1, f"geglu lean ln-fold {M}x{N}x{C} parts={parts}", idx=idx)
    else:
        p64, m64 = gemm_ref(h, r16(w), b)
        acc = U32 * (C + 1) * m64
        assert_elementwise(outs[0], *geglu_ref_bound(p64[:, :H], acc[:, :H], p64[:, H:], acc[:, H:]), f"geglu lean {M}x{N}x{C}",
                           ("row", "col"))


@pytest.mark.parametrize("M,C,epi", [(16384, 640, 1), (65536, 320, 0), (16384, 640, 0), (4096, 1280, 1)])
def test_layernorm_fold_gemms_are_run_to_run_deterministic_at_bench_shapes(sdlib, M, C, epi):
    """The LayerNorm-fold consumers at the bench's own shapes (several work items per workgroup, cold caches on the first
    launch): six launches into six fresh tensors give the same bits.  Round 4 found the first launch of the 8-wave GEGLU
    instantiation differing from the later ones in a few dozen elements (a timing-dependent hazard around the per-wave
    (mean, rstd) exchange through LDS, csrc/gemm_lean.hip); the small-shape reproducibility test of test_unet_gpu.py never
    reaches these grids."""
    g = torch.Generator(device="cuda").manual_seed(M + C + epi)
    N = 8 * C if epi else 3 * C
    H = N // 2 if epi else N
    x = (torch.randn(M, C, device="cuda", generator=g) * 1.5 + 0.4).to(torch.bfloat16)
    w = (torch.randn(N, C, device="cuda", generator=g) / math.sqrt(C)).to(torch.bfloat16)
    c1, c2 = torch.randn(N, device="cuda", generator=g), torch.randn(N, device="cuda", generator=g)
    parts = 2 * (C // 160)
    xf = x.float().view(M, parts, C // parts)
    rs = torch.stack([xf.sum(2), (xf * xf).sum(2)], dim=2).permute(1, 0, 2).contiguous()
    x, w, c1, c2, rs = G(x), G(w), G(c1), G(c2), G(rs)
    outs = [OUT((M, H)) for _ in range(6)]
    for out in outs:
        _lib.check(sdlib.sd_op_gemm_ln(stream(), P(x), C, P(w), P(c1), P(c2), P(rs), parts, 1e-5, P(out), H, M, N, C, epi))
    torch.cuda.synchronize()
    check_guards()
    assert torch.isfinite(outs[0].float()).all()
    for out in outs[1:]:
        assert torch.equal(out, outs[0])
    # per element on the first and last 256 rows (the fp64 reference of all rows would dominate the suite's time);
    # epi 1 packs [16 value | 16 gate] in the weight's row order, which the reference here follows
    rows = torch.cat([torch.arange(256), torch.arange(M - 256, M)])
    idx = None
    if epi:
        idx = torch.tensor([(q // 32) * 16 + q % 32 if q % 32 < 16 else H + (q // 32) * 16 + q % 32 - 16 for q in range(N)])
    ln_fold_elementwise(outs[0], x, w, c1, c2, rs, epi, f"gemm_ln bench {M}x{N}x{C} epi{epi}", rows=rows, idx=idx)


@pytest.mark.parametrize("rows,C", [(300, 320), (77, 640), (1024, 1280)])
def test_layernorm(sdlib, rows, C):
    """Per element and by count (assert_flip_budget against the two-pass fp32 restatements of the kernels' formula); measured
    flips / F_ref / numel: 3 / 4 / 96000, 1 / 5 / 49280, 47 / 153 / 1310720."""
    g = torch.Generator().manual_seed(rows)
    x = r16(torch.randn(rows, C, generator=g) * 3 + 1)
    gamma, beta = torch.randn(C, generator=g), torch.randn(C, generator=g)
    ref = F.layer_norm(x, (C,), gamma, beta, 1e-5)
    out = OUT((rows, C))
    _lib.check(sdlib.sd_op_layernorm(stream(), P(G(x, torch.bfloat16)), P(G(gamma)),
                                     P(G(beta)), P(out), rows, C, 1e-5))
    torch.cuda.synchronize()
    check_guards()
    assert rel_l2(out, ref) < TOL
    n64, nb = norm_ref_bound(x, gamma, beta, C, 1e-5, False)
    assert_elementwise(out, n64, nb, f"layernorm {rows}x{C}", ("row", "c"))
    assert_flip_budget(out, n64, ln_restatements(x, gamma, beta, 1e-5), "bf16", f"layernorm {rows}x{C}", acc_bound=nb - ulp_bf16(n64))


@pytest.mark.parametrize("B,heads,Nq,Nk,D,spike", [
    (2, 8, 256, 256, 40, False),
    (1, 8, 300, 300, 40, True),     # ragged tiles + a spiked key that forces the online-max rescale
    (2, 8, 256, 77, 40, False),     # prompt cross-attention
    (1, 8, 128, 128, 80, False),
    (2, 8, 64, 77, 80, False),
    (1, 8, 64, 64, 160, True),
    (2, 8, 16, 77, 160, False),
    (1, 8, 4096, 4096, 40, False),  # the SD-1.5 64x64 self-attention shape
    (1, 8, 256, 192, 80, False),    # attn_pipe80_kernel (round 5): odd tile count, the minimum of three tiles
    (2, 8, 1024, 1024, 80, True),   # ... the SD-1.5 32x32 self-attention shape, a spiked key in the last tile
    (1, 8, 200, 320, 80, True),     # ... ragged query count (the last workgroup's waves past Nq), five tiles
])
def test_attention(sdlib, B, heads, Nq, Nk, D, spike):
    g = torch.Generator().manual_seed(Nq + D)
    C = heads * D
    q = r16(torch.randn(B, Nq, C, generator=g))
    k = r16(torch.randn(B, Nk, C, generator=g))
    v = r16(torch.randn(B, Nk, C, generator=g))
    if spike:  # one late key dominates -> running max jumps in the last tile
        k[:, Nk - 3] = k[:, Nk - 3] * 6
    qh = q.view(B, Nq, heads, D).transpose(1, 2)
    kh = k.view(B, Nk, heads, D).transpose(1, 2)
    vh = v.view(B, Nk, heads, D).transpose(1, 2)
    ref = F.scaled_dot_product_attention(qh, kh, vh).transpose(1, 2).reshape(B, Nq, C)
    # pack K|V side by side like the fused projections do
    kv = G(torch.cat([k, v], dim=-1).contiguous(), torch.bfloat16)
    qd = G(q, torch.bfloat16)
    out = OUT((B, Nq, C))
    kvp = P(kv)
    _lib.check(sdlib.sd_op_attention(stream(), P(qd), C, kvp, 2 * C, kvp + 2 * C, 2 * C, P(out), C, B,
                                     heads, Nq, Nk, D, 1.0 / math.sqrt(D)))
    torch.cuda.synchronize()
    check_guards()
    assert rel_l2(out, ref) < 1e-2   # P is rounded to bf16 before PV
    attention_elementwise(out, q, k, v, heads, D, f"attention B={B} {Nq}x{Nk} d{D}")




@pytest.mark.parametrize("Nk,spikes", [(512, ((70, 6.0), (300, 14.0), (509, 40.0))), (1024, ((5, 30.0), (640, 3.0))),
                                       (256, ((250, 25.0),))])
def test_attention_pipelined_kernel_moves_its_stale_reference(sdlib, Nk, spikes):
    """The 64x64-level kernel (d = 40, key count a multiple of 64) keeps a STALE softmax reference M inside the QK^T product
    and only moves it when a tile's scores exceed it by 2^8: keys scaled up mid-sequence, in the second tile and in the last
    one force that path (and the O rescale) several times per query, with jumps from a few to hundreds of log2 units."""
    g = torch.Generator().manual_seed(Nk)
    B, heads, D, Nq = 1, 8, 40, 256
    C = heads * D
    q = r16(torch.randn(B, Nq, C, generator=g))
    k = r16(torch.randn(B, Nk, C, generator=g))
    v = r16(torch.randn(B, Nk, C, generator=g))
    for pos, f in spikes:
        k[:, pos] = r16(k[:, pos] * f)
    qh, kh, vh = (t.view(B, -1, heads, D).transpose(1, 2) for t in (q, k, v))
    ref = F.scaled_dot_product_attention(qh, kh, vh).transpose(1, 2).reshape(B, Nq, C)
    kv = G(torch.cat([k, v], dim=-1).contiguous(), torch.bfloat16)
    out = OUT((B, Nq, C))
    kvp = P(kv)
    _lib.check(sdlib.sd_op_attention(stream(), P(G(q, torch.bfloat16)), C, kvp, 2 * C, kvp + 2 * C, 2 * C, P(out), C, B,
                                     heads, Nq, Nk, D, 1.0 / math.sqrt(D)))
    torch.cuda.synchronize()
    check_guards()
    assert torch.isfinite(out.float()).all()
    assert rel_l2(out, ref) < 1e-2
    attention_elementwise(out, q, k, v, heads, D, f"attention stale-reference Nk={Nk}")


def _dominant_key_case(g, B, heads, D, Nq, Nk, spikes):
    """Queries with a common component u, keys f * u at the given positions: key `pos` then scores ~ 18 f log2 units above
    everything before it for EVERY query (q . u = 2 D +- sqrt(D)), as the BOS key of a real prompt / an outlier channel of
    a real checkpoint does.  Escalating factors make each spike exceed the previous maximum by >= 150 log2 units."""
    C = heads * D
    u = torch.ones(C)
    q = r16(torch.randn(B, Nq, C, generator=g) + 2.0 * u)
    k = r16(torch.randn(B, Nk, C, generator=g))
    v = r16(torch.randn(B, Nk, C, generator=g))
    for pos, f in spikes:
        k[:, pos] = r16(f * u * (math.sqrt(40.0 / D)) + 0.1 * k[:, pos])     # ~ the same log2 jump per unit of f for every D
    return q, k, v


@pytest.mark.parametrize("D,Nk,spikes", [
    (40, 77, ((5, 13.0), (41, 26.0), (76, 39.0))),          # attn_dma_kernel<40>: the 77-key prompt shape, both lane halves
    (40, 200, ((9, 13.0), (68, 26.0), (197, 39.0))),        # attn_dma_kernel<40>: key count not a multiple of 64
    (40, 512, ((13, 13.0), (300, 26.0), (509, 39.0))),      # attn_pipe40_kernel (stale reference): jumps of >= 150 log2 units
    (80, 256, ((5, 13.0), (130, 26.0), (251, 39.0))),       # attn_kernel<80>
    (80, 1024, ((9, 13.0), (520, 26.0), (1021, 39.0))),
    (160, 64, ((4, 13.0), (25, 26.0), (61, 39.0))),         # attn_kernel<160>
    (160, 256, ((12, 13.0), (100, 26.0), (255, 39.0))),
])
def test_attention_running_maximum_survives_dominant_keys_in_either_lane_half(sdlib, D, Nk, spikes):
    """Rounds 1-2 shipped a running maximum that covered only HALF of the keys of a tile (the other lane of a query's lane
    pair, csrc/attention.hip::half_pair_max): an exact softmax still, so every parity test passed, until a score in the
    uncovered half sat > 128 log2 units above it and exp2 overflowed.  Every flash-attention kernel (d = 40 DMA / pipelined,
    d = 80, d = 160) is driven here with dominant keys at early / middle / last positions whose index covers both values of
    bits 2 and 3 (the accumulator rows one lane of the pair owns), each >= 150 log2 units above the maximum before it:
    finite, and rel-L2 <= 1e-2 against fp32 SDPA (src/models.py:227-235: real prompts have a dominant BOS key)."""
    g = torch.Generator().manual_seed(D * 1000 + Nk)
    B, heads, Nq = 1, 8, 256
    C = heads * D
    q, k, v = _dominant_key_case(g, B, heads, D, Nq, Nk, spikes)
    qh, kh, vh = (t.view(B, -1, heads, D).transpose(1, 2) for t in (q, k, v))
    scale = 1.0 / math.sqrt(D)
    s = (qh @ kh.transpose(-1, -2)) * scale * 1.4426950408889634
    for pos, _ in spikes:                                          # the construction really produces the jumps it claims
        assert (s[..., pos] - s[..., :pos].amax(-1)).min() > 150.0
    ref = F.scaled_dot_product_attention(qh, kh, vh).transpose(1, 2).reshape(B, Nq, C)
    kv = G(torch.cat([k, v], dim=-1).contiguous(), torch.bfloat16)
    out = OUT((B, Nq, C))
    kvp = P(kv)
    _lib.check(sdlib.sd_op_attention(stream(), P(G(q, torch.bfloat16)), C, kvp, 2 * C, kvp + 2 * C, 2 * C, P(out), C, B,
                                     heads, Nq, Nk, D, scale))
    torch.cuda.synchronize()
    check_guards()
    assert torch.isfinite(out.float()).all()
    assert rel_l2(out, ref) < 1e-2
    attention_elementwise(out, q, k, v, heads, D, f"attention dominant keys d{D} Nk={Nk}")


def test_clip_attention_with_a_dominant_bos_key(sdlib):
    """The CLIP text tower's causal attention (csrc/clip.hip, 77 tokens): every query sees key 0 (BOS) scoring ~700 log2
    units above the rest, as real CLIP text models do; exact two-pass softmax -> finite and equal to fp32 SDPA."""
    g = torch.Generator().manual_seed(77)
    B, L, heads, D = 2, 77, 12, 64
    H = heads * D
    q, k, v = _dominant_key_case(g, B, heads, D, L, L, ((0, 40.0),))
    qkv = G(torch.cat([q, k, v], dim=-1).contiguous(), torch.bfloat16)
    out = OUT((B * L, H))
    _lib.check(sdlib.sd_op_clip_attention(stream(), P(qkv), P(out), B, L, H, heads))
    torch.cuda.synchronize()
    check_guards()
    attention_elementwise(out, q, k, v, heads, D, "attention clip causal", causal=True)
    qh, kh, vh = (t.view(B, L, heads, D).transpose(1, 2) for t in (q, k, v))
    ref = F.scaled_dot_product_attention(qh, kh, vh, is_causal=True).transpose(1, 2).reshape(B * L, H)
    assert torch.isfinite(out.float()).all()
    assert rel_l2(out, ref) < TOL


def test_qkv_projection_and_attention_head_major(sdlib):
    """The 64x64 level's pair: the q|k|v projection stores K and V head-major ([which][sample][head][token][40]) and the
    self-attention reads them as contiguous 5 KiB tiles; against linear + scaled_dot_product_attention."""
    g = torch.Generator().manual_seed(3)
    B, N, C, H, D = 2, 4096, 320, 8, 40      # M = 8192 rows: the smallest problem that runs on 128-row GEMM tiles
    M = B * N
    x = r16(torch.randn(M, C, generator=g))
    w = r16(torch.randn(3 * C, C, generator=g) / math.sqrt(C))
    qkv = r16(x @ w.t())
    q = OUT((M, C))
    kv = OUT((2, B, H, N, D))
    _lib.check(sdlib.sd_op_gemm_qkv_headmajor(stream(), P(G(x, torch.bfloat16)), C, P(G(w, torch.bfloat16)), P(q), P(kv), M, C, N, C))
    torch.cuda.synchronize()
    assert rel_l2(q, qkv[:, :C]) < TOL
    for which in (0, 1):
        want = qkv[:, (1 + which) * C:(2 + which) * C].view(B, N, H, D).permute(0, 2, 1, 3)
        assert rel_l2(kv[which], want) < TOL
    r64, b64 = gemm_bound(x, w)
    assert_elementwise(q, r64[:, :C], b64[:, :C], "gemm qkv head-major q", ("row", "col"))
    for which in (0, 1):
        sl = slice((1 + which) * C, (2 + which) * C)
        assert_elementwise(kv[which], r64[:, sl].reshape(B, N, H, D).permute(0, 2, 1, 3), b64[:, sl].reshape(B, N, H, D).permute(0, 2, 1, 3),
                           f"gemm qkv head-major {'kv'[which]}", ("b", "head", "token", "d"))
    out = OUT((B, N, C))
    # K and V each in their own poisoned allocation (an over-read of K must not land in V)
    _lib.check(sdlib.sd_op_attention_headmajor(stream(), P(q), C, P(G(kv[0])), P(G(kv[1])), P(out), C, B, H, N, N, D, 1.0 / math.sqrt(D)))
    torch.cuda.synchronize()
    qh = q.float().cpu().view(B, N, H, D).transpose(1, 2)
    ref = F.scaled_dot_product_attention(qh, kv[0].float().cpu(), kv[1].float().cpu()).transpose(1, 2).reshape(B, N, C)
    assert rel_l2(out, ref) < 1e-2   # P is rounded to bf16 before PV
    # and the token-major call on the same data gives the same result bit for bit (only the DMA source addresses differ)
    ktm = G(kv[0].permute(0, 2, 1, 3).reshape(B, N, C).contiguous())
    vtm = G(kv[1].permute(0, 2, 1, 3).reshape(B, N, C).contiguous())
    out2 = OUT((B, N, C))
    _lib.check(sdlib.sd_op_attention(stream(), P(q), C, P(ktm), C, P(vtm), C, P(out2), C, B, H, N, N, D, 1.0 / math.sqrt(D)))
    torch.cuda.synchronize()
    check_guards()
    assert torch.equal(out, out2)
    attention_elementwise(out, q.view(B, N, C), ktm, vtm, H, D, "attention head-major 2x4096 d40")


def test_conv_in_out(sdlib):
    g = torch.Generator().manual_seed(11)
    Bs, B, H, C = 2, 4, 16, 320
    x = torch.randn(Bs, 4, H, H, generator=g)
    w = torch.randn(C, 4, 3, 3, generator=g) / 6
    b = torch.randn(C, generator=g)
    ref = F.conv2d(torch.cat([x, x]), w, b, padding=1)
    wt = G(w.reshape(C, 36).t().contiguous())
    out = OUT((B, H, H, C))
    _lib.check(sdlib.sd_op_conv_in(stream(), P(G(x)), Bs, P(wt), P(G(b)), P(out), B, H, H, 4, C))
    torch.cuda.synchronize()
    check_guards()
    assert rel_l2(out.permute(0, 3, 1, 2), ref) < TOL
    r64, m64 = conv3x3_nhwc_ref(torch.cat([x, x]), w, b)          # fp32 inputs and weights: fp32 products (one more rounding)
    assert_elementwise(out, r64, linear_bound(r64, m64, 2 * 36 + 1), "conv_in", NHWC)
    # conv_out
    y = r16(torch.randn(B, C, H, H, generator=g))
    w2 = r16(torch.randn(4, C, 3, 3, generator=g) / math.sqrt(9 * C))
    b2 = torch.randn(4, generator=g)
    ref2 = F.conv2d(y, w2, b2, padding=1)
    yd = G(y.permute(0, 2, 3, 1).contiguous(), torch.bfloat16)
    wp = G(w2.permute(0, 2, 3, 1).contiguous(), torch.bfloat16)
    out2 = OUT((B, 4, H, H), torch.float32)
    _lib.check(sdlib.sd_op_conv_out(stream(), P(yd), P(wp), P(G(b2)), P(out2), B, H, H, C, 4))
    torch.cuda.synchronize()
    check_guards()
    assert rel_l2(out2, ref2) < 1e-5
    r64, m64 = conv3x3_nhwc_ref(y, w2, b2)
    assert_elementwise(out2.permute(0, 2, 3, 1), r64, linear_bound(r64, m64, 9 * C + 1, torch.float32), "conv_out", NHWC)


@pytest.mark.parametrize("B,H,W,C,Cout", [
    (2, 64, 64, 320, 4),      # the UNet's conv_out
    (1, 24, 40, 128, 3),      # the VAE decoder's: 3 channels, non-square image
    (3, 5, 7, 64, 4),         # 105 pixels: ragged last tile, every pixel near a border
])
def test_conv_out_matrix_core_kernel(sdlib, B, H, W, C, Cout):
    g = torch.Generator().manual_seed(H * W + C)
    y = r16(torch.randn(B, C, H, W, generator=g))
    w2 = r16(torch.randn(Cout, C, 3, 3, generator=g) / math.sqrt(9 * C))
    b2 = torch.randn(Cout, generator=g)
    ref = F.conv2d(y, w2, b2, padding=1)
    yd = G(y.permute(0, 2, 3, 1).contiguous(), torch.bfloat16)
    wp = G(w2.permute(0, 2, 3, 1).contiguous(), torch.bfloat16)
    out = OUT((B, Cout, H, W), torch.float32)
    _lib.check(sdlib.sd_op_conv_out(stream(), P(yd), P(wp), P(G(b2)), P(out), B, H, W, C, Cout))
    torch.cuda.synchronize()
    check_guards()
    assert rel_l2(out, ref) < 1e-5
    r64, m64 = conv3x3_nhwc_ref(y, w2, b2)
    assert_elementwise(out.permute(0, 2, 3, 1), r64, linear_bound(r64, m64, 9 * C + 1, torch.float32),
                       f"conv_out matrix-core B={B} {H}x{W} {C}->{Cout}", NHWC)


def test_time_embedding(sdlib):
    g = torch.Generator().manual_seed(5)
    w1 = r16(torch.randn(1280, 320, generator=g) / 18); b1 = torch.randn(1280, generator=g)
    w2 = r16(torch.randn(1280, 1280, generator=g) / 36); b2 = torch.randn(1280, generator=g)
    for t in (981.0, 501.0, 1.0):
        half = 160
        f = torch.exp(-math.log(10000.0) * torch.arange(half, dtype=torch.float32) / half)
        emb = torch.cat([torch.cos(t * f), torch.sin(t * f)])
        ref = F.linear(F.silu(F.linear(emb, w1, b1)), w2, b2)
        scratch = OUT((320 + 1280,), torch.float32)
        out = OUT((1280,), torch.float32)
        _lib.check(sdlib.sd_op_time_embedding(stream(), t, P(G(w1, torch.bfloat16)), P(G(b1)),
                                              P(G(w2, torch.bfloat16)), P(G(b2)), P(scratch),
                                              P(out), 320, 1280))
        torch.cuda.synchronize()
        check_guards()
        assert rel_l2(out, ref) < 1e-4
        # each stage from the kernel's own stored intermediate: sinusoid (fp32 expf of the frequency exponent, t f rounded,
        # cosf / sinf: <= 16 u |t f| of phase + 2^-21), GEMV + bias, SiLU (a few ulp) + GEMV + bias
        fd = torch.exp(-math.log(10000.0) * torch.arange(half, dtype=torch.float64) / half)
        e64 = torch.cat([torch.cos(t * fd), torch.sin(t * fd)])
        assert_elementwise(scratch[:320], e64, 16 * U32 * t * torch.cat([fd, fd]) + 2.0 ** -21, f"time embedding sinusoid t={t}")
        emb_k, h_k = scratch[:320].double().cpu(), scratch[320:].double().cpu()
        r1, m1 = gemm_ref(emb_k[None], w1, b1)
        assert_elementwise(scratch[320:], r1[0], linear_bound(r1[0], m1[0], 321, torch.float32), f"time embedding linear_1 t={t}")
        sh = F.silu(h_k)
        r2, m2 = gemm_ref(sh[None], w2, b2)
        assert_elementwise(out, r2[0], linear_bound(r2[0], m2[0], 1281 + 8, torch.float32), f"time embedding linear_2 t={t}")


def test_sched_step_kernel(sdlib):
    import ctypes
    g = torch.Generator().manual_seed(9)
    n = 2 * 4 * 16 * 16
    eps = torch.randn(2 * n, generator=g); x = torch.randn(n, generator=g)
    m1 = torch.randn(n, generator=g); m2 = torch.randn(n, generator=g); z = torch.randn(n, generator=g)
    m3 = torch.randn(n, generator=g)
    coef = [0.9, -0.3, 0.2, -0.1, 0.05, 1.3, -0.7, 0.4, 0.6, 0.15]
    gs = 7.5
    e = eps[:n] + gs * (eps[n:] - eps[:n])
    prev = coef[0] * x + coef[1] * e + coef[2] * m1 + coef[3] * m2 + coef[9] * m3 + coef[4] * z
    y2 = coef[5] * x + coef[6] * e
    mo = coef[7] * x + coef[8] * e
    d = [dev(t) for t in (eps, x, m1, m2, z)]
    o = [torch.zeros(n, device="cuda") for _ in range(3)]
    carr = (ctypes.c_float * 10)(*coef)
    _lib.check(sdlib.sd_sched_step(stream(), P(d[0]), 1, gs, P(d[1]), P(d[2]), P(d[3]), P(m3),
                                   P(d[4]), P(o[0]), P(o[1]), P(o[2]), carr, n))
    torch.cuda.synchronize()
    for got, ref in zip(o, (prev, y2, mo)):
        assert torch.allclose(got.cpu(), ref, rtol=1e-5, atol=1e-5)




@pytest.mark.parametrize("B,rows,N,K,epi", [(3, 256, 640, 320, 2), (2, 128, 320, 640, 0), (4, 1024, 640, 640, 2)])
def test_gemm_batched_weights_and_grouped_softmax(sdlib, B, rows, N, K, epi):
    """Per-sample W (+ residual / bias) and the softmax-over-77-of-80 epilogue: the two GEMMs of the folded
    prompt cross-attention."""
    g = torch.Generator().manual_seed(rows + N)
    x = r16(torch.randn(B * rows, K, generator=g))
    w = r16(torch.randn(B, N, K, generator=g) / math.sqrt(K) * (4.0 if epi else 1.0))
    xb = x.view(B, rows, K)
    ref = torch.einsum("brk,bnk->brn", xb, w)
    if epi == 2:
        s = ref.view(B, rows, N // 80, 80)
        p = torch.zeros_like(s)
        p[..., :77] = torch.softmax(s[..., :77], dim=-1)
        ref = p.view(B * rows, N)
        bias = res = None
    else:
        bias = torch.randn(N, generator=g)
        res = r16(torch.randn(B * rows, N, generator=g))
        ref = ref.reshape(B * rows, N) + bias + res
    out = OUT((B * rows, N))
    _lib.check(sdlib.sd_op_gemm_batched(stream(), P(G(x, torch.bfloat16)), K, P(G(w, torch.bfloat16)), N * K, rows,
                                        P(G(bias)) if bias is not None else None,
                                        P(G(res, torch.bfloat16)) if res is not None else None, N, P(out), N,
                                        B * rows, N, K, epi, 77 if epi else 0))
    torch.cuda.synchronize()
    check_guards()
    assert rel_l2(out, ref) < TOL
    s64 = torch.einsum("brk,bnk->brn", xb.double(), w.double())
    m64 = torch.einsum("brk,bnk->brn", xb.double().abs(), w.double().abs())
    if epi == 2:
        grouped_softmax_elementwise(out, s64.reshape(B * rows, N), U32 * K * m64.reshape(B * rows, N), 77,
                                     f"gemm batched softmax B={B} rows={rows} K={K}")
    else:
        r64 = s64.reshape(B * rows, N) + bias.double() + res.double()
        m64 = m64.reshape(B * rows, N) + bias.double().abs() + res.double().abs()
        assert_elementwise(out, r64, linear_bound(r64, m64, K + 2), f"gemm batched B={B} rows={rows} {N}x{K}", ("row", "col"))

    if epi == 2:
        o = out.float().view(B * rows, N // 80, 80)
        assert (o[..., 77:] == 0).all() and (o.sum(-1) - 1).abs().max() < 2e-2


@pytest.mark.parametrize("B,rows,C,offset", [(3, 256, 1280, 0.8), (2, 128, 640, 0.0)])
def test_gemm_per_sample_softmax_with_layernorm_folded(sdlib, B, rows, C, offset):
    """First GEMM of the two-GEMM prompt cross-attention (16x16 level) with the block's norm2 folded in: P = softmax_77 over
    every head's 80 key slots of LayerNorm(x) . A^T, computed from the UN-normalised rows, their (sum, sum of squares) partials,
    the gamma-scaled per-sample operand and per-sample c1 / c2 vectors.  Against LayerNorm + einsum + softmax in fp64."""
    g = torch.Generator().manual_seed(rows + C)
    N, L, M = 640, 77, B * rows
    x = r16(torch.randn(M, C, generator=g) * 0.8 + offset)
    gamma, beta = 1.0 + 0.3 * torch.randn(C, generator=g), 0.3 * torch.randn(C, generator=g)
    w = (torch.randn(B, N, C, generator=g) / math.sqrt(C) * 3.0).double()
    wg = w * gamma.double()
    wln = r16((wg - wg.mean(-1, keepdim=True)).float())                  # centred, as the packer does for A^T
    c1 = wln.double().sum(-1).float().contiguous()                          # [B, N]: what the centring leaves after rounding
    c2 = (w @ beta.double()).float().contiguous()
    parts = 2 * ((C + 159) // 160)
    xs = x.double().view(M, C // 80, 80)
    rs = torch.stack([xs.sum(-1), (xs * xs).sum(-1)], -1).permute(1, 0, 2).float().contiguous()
    mean = x.double().mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(x.double().var(-1, unbiased=False, keepdim=True) + 1e-5)
    xn = ((x.double() - mean) * rstd * gamma.double() + beta.double()).view(B, rows, C)
    S = torch.einsum("brk,bnk->brn", xn, w).view(B, rows, N // 80, 80)
    ref = torch.zeros_like(S)
    ref[..., :L] = torch.softmax(S[..., :L], dim=-1)
    ref = ref.view(M, N).float()
    out = OUT((M, N))
    _lib.check(sdlib.sd_op_gemm_batched_softmax_ln(stream(), P(G(x, torch.bfloat16)), C, P(G(wln, torch.bfloat16)), N * C, rows,
                                                   P(out), N, M, N, C, L, P(G(rs)), parts, P(G(c1)), P(G(c2)), 1e-5))
    torch.cuda.synchronize()
    check_guards()
    tot = rs.double().sum(0)
    zs, dzs = zip(*(ln_fold_ref_bound(x[b * rows:(b + 1) * rows], wln[b], c1[b], c2[b], tot[b * rows:(b + 1) * rows, 0],
                                      tot[b * rows:(b + 1) * rows, 1], 1e-5) for b in range(B)))
    grouped_softmax_elementwise(out, torch.cat(zs), torch.cat(dzs), L, f"gemm batched softmax+ln B={B} rows={rows} C={C}")
    e = rel_l2(out, ref)
    print(f"softmax GEMM + norm2 B={B} rows={rows} C={C} offset={offset}: {e:.3e}")
    assert e < 1e-2                               # (bf16 rounding of the centred operand and of the probabilities)
    o = out.float().view(M, N // 80, 80)
    assert (o[..., L:] == 0).all() and (o.sum(-1) - 1).abs().max() < 2e-2





@pytest.mark.parametrize("B,hw,C,spike", [(2, 256, 320, False), (1, 1024, 640, True), (3, 128, 1280, False), (2, 4096, 320, False),
                                          (2, 256, 320, 40.0), (1, 128, 1280, 40.0),
                                          (10, 4096, 320, False), (36, 1024, 640, True)])   # more token blocks than CUs: several rounds of workgroups
def test_xattn_fused(sdlib, B, hw, C, spike):
    """Fused prompt cross-attention (xattn.hip; src/models.py:227-235 -> diffusers Attention over the 77 prompt keys):
    Y = R + to_out(softmax(to_q(X) K^T / sqrt(d)) V) + b in ONE launch with A_h = scale W_q,h^T K_h^T and
    B_h = V_h W_o,h^T precomputed per prompt.  Checked against (i) the same folded form evaluated in fp32 from the
    bf16-rounded A / B (kernel arithmetic: probabilities are rounded to bf16 before the second product -> 8e-3) and
    (ii) F.scaled_dot_product_attention + linears on the unfolded weights (the formulation itself, incl. the
    bf16 rounding of A and B: 2e-2)."""
    g = torch.Generator().manual_seed(B * 1000 + hw + C)
    H, L, d = 8, 77, C // 8
    M = B * hw
    x = r16(torch.randn(M, C, generator=g))
    r = r16(torch.randn(M, C, generator=g))
    wq, wo = (torch.randn(C, C, generator=g) / math.sqrt(C) for _ in range(2))
    wk, wv = (torch.randn(C, 768, generator=g) / math.sqrt(768) for _ in range(2))
    bo = torch.randn(C, generator=g)
    ctx = torch.randn(B, L, 768, generator=g)
    if spike is True:
        ctx[0, 5] *= 6.0                      # one dominant key: exercises the max subtraction
    elif spike:
        # a BOS-like key: EVERY query of every head scores it far above the other 76 (real prompts: key 0), hundreds of
        # log2 units -- the probabilities collapse onto it and nothing may overflow on the way.  Queries share the component
        # W_q 1 (x = noise + 1); the key is made parallel to it: K_0 = wk ctx_0 ~ c W_q 1 -> score_h ~ c sqrt(d) +- c.
        x = r16(x + 1.0)
        ctx[:, 0] = spike * (torch.linalg.pinv(wk) @ (wq @ torch.ones(C)))
    K, V = ctx @ wk.t(), ctx @ wv.t()         # [B, L, C]
    scale = 1.0 / math.sqrt(d)
    At = torch.zeros(B, H * 80, C)
    Bn = torch.zeros(B, H * 80, C)            # natural key order, [key slot][channel]
    for hh in range(H):
        sl = slice(hh * d, (hh + 1) * d)
        At[:, hh * 80: hh * 80 + L] = scale * K[:, :, sl] @ wq[sl, :]
        Bn[:, hh * 80: hh * 80 + L] = V[:, :, sl] @ wo[:, sl].t()
    At, Bn = r16(At), r16(Bn)
    # (i) folded reference from the rounded operands
    xs = x.view(B, hw, C)
    S = torch.einsum("bmc,bkc->bmk", xs, At).view(B, hw, H, 80)
    S[..., L:] = float("-inf")
    Pm = torch.softmax(S, dim=-1).view(B, hw, H * 80)
    ref_fold = (r.view(B, hw, C) + torch.einsum("bmk,bkc->bmc", Pm, Bn) + bo).view(M, C)
    # (ii) the unfolded attention
    q = (xs @ wq.t()).view(B, hw, H, d).transpose(1, 2)
    kk, vv = (t.view(B, L, H, d).transpose(1, 2) for t in (K, V))
    o = F.scaled_dot_product_attention(q, kk, vv).transpose(1, 2).reshape(B, hw, C)
    ref_attn = (r.view(B, hw, C) + o @ wo.t() + bo).view(M, C)
    # Bw: [B][C][640] with bits 2 and 3 of the key slot swapped inside every group of 16
    slot = torch.arange(H * 80)
    perm = (slot & ~12) | ((slot & 4) << 1) | ((slot & 8) >> 1)
    Bw = torch.zeros(B, C, H * 80)
    Bw[:, :, perm] = Bn.transpose(1, 2)
    # tiled operand layouts (one contiguous KiB per 16-row x 64-byte DMA piece): A^T [C/32][640][32], Bw [C/32][20][32][32]
    At_t = At.view(B, H * 80, C // 32, 32).permute(0, 2, 1, 3).contiguous()
    Bw_t = Bw.view(B, C // 32, 32, 20, 32).permute(0, 1, 3, 2, 4).contiguous()
    xd_, rd_, Ad_, Bd_, bod = G(x, torch.bfloat16), G(r, torch.bfloat16), G(At_t, torch.bfloat16), G(Bw_t, torch.bfloat16), G(bo)
    out = OUT((M, C))
    _lib.check(sdlib.sd_op_xattn_fused(stream(), P(xd_), P(rd_), P(out), P(Ad_), P(Bd_), P(bod), M, C, hw, L))
    torch.cuda.synchronize()
    e1, e2 = rel_l2(out, ref_fold), rel_l2(out, ref_attn)
    print(f"xattn fused B={B} hw={hw} C={C}: vs folded fp32 {e1:.3e}, vs SDPA + linears {e2:.3e}")
    assert torch.isfinite(out.float()).all()
    assert e1 < 8e-3 and e2 < 2e-2
    # the same launch also delivers the LayerNorm partials of its stored rows (norm3 folded into the GEGLU projection)
    parts = sdlib.sd_op_ln_partials(1, M, C)
    rs = OUT((parts, M, 2), torch.float32)
    out2 = OUT((M, C))
    _lib.check(sdlib.sd_op_xattn_fused_rowstats(stream(), P(xd_), P(rd_), P(out2), P(Ad_), P(Bd_), P(bod), M, C, hw, L, P(rs)))
    torch.cuda.synchronize()
    check_guards()
    assert torch.equal(out2, out)
    sel = sample_rows(B, hw)
    x64, A64 = x.double().view(B, hw, C)[sel], At.double()[sel]
    xattn_elementwise(out.view(B, hw, C)[sel], torch.einsum("bmc,bkc->bmk", x64, A64), torch.einsum("bmc,bkc->bmk", x64.abs(), A64.abs()),
                       U32 * (C + 2), Bn[sel], r.view(B, hw, C)[sel], bo, L, f"xattn fused B={B} hw={hw} C={C}")
    tot = rs.sum(0).cpu()
    o64 = out.double().cpu()
    assert torch.allclose(tot[:, 0].double(), o64.sum(1), rtol=1e-4, atol=1e-2)
    assert torch.allclose(tot[:, 1].double(), (o64 * o64).sum(1), rtol=1e-4, atol=1e-2)


@pytest.mark.parametrize("B,hw,C,offset,dup", [(2, 256, 320, 0.0, False), (1, 1024, 640, 1.5, False), (2, 128, 1280, 0.5, False),
                                               (4, 4096, 320, 1.0, True)])
def test_xattn_fused_with_norm2_folded(sdlib, B, hw, C, offset, dup):
    """The block's norm2 folded into the fused cross-attention (diffusers BasicTransformerBlock: attn2(norm2(h)) + h, reached
    from src/models.py:227-235): the kernel reads the UN-normalised rows, takes rstd of a row from its producer's (sum, sum of
    squares) partials, and the operand A is scaled by gamma and CENTRED over the channel so that the row mean drops out
    (sum_c (x_c - m) w_c = sum_c x_c (w_c - mean(w))); the beta term is a per-key-slot constant c2.  Against (i) the same
    formula in fp64 from the rounded operands and (ii) LayerNorm + F.scaled_dot_product_attention + linears.  offset: rows
    with |mean| ~ sigma (the centring carries the whole subtraction); dup: a CFG pair replicated after the producer ran
    (row m reads partials row m % ln_rows)."""
    g = torch.Generator().manual_seed(B * 1000 + hw + C + 7)
    H, L, d = 8, 77, C // 8
    Bu = B // 2 if dup else B                  # distinct samples of rows
    M, Mu = B * hw, Bu * hw
    xu = r16(torch.randn(Mu, C, generator=g) * 0.7 + offset + 0.3 * torch.randn(Mu, 1, generator=g))
    x = torch.cat([xu, xu]) if dup else xu
    r = r16(torch.randn(M, C, generator=g))
    gamma, beta = 1.0 + 0.3 * torch.randn(C, generator=g), 0.3 * torch.randn(C, generator=g)
    wq, wo = (torch.randn(C, C, generator=g) / math.sqrt(C) for _ in range(2))
    wk, wv = (torch.randn(C, 768, generator=g) / math.sqrt(768) for _ in range(2))
    bo = torch.randn(C, generator=g)
    ctx = torch.randn(B, L, 768, generator=g)
    ctx[0, 5] *= 4.0
    K, V = ctx @ wk.t(), ctx @ wv.t()
    scale = 1.0 / math.sqrt(d)
    At = torch.zeros(B, H * 80, C, dtype=torch.float64)
    Bn = torch.zeros(B, H * 80, C)
    for hh in range(H):
        sl = slice(hh * d, (hh + 1) * d)
        At[:, hh * 80: hh * 80 + L] = (scale * K[:, :, sl] @ wq[sl, :]).double()
        Bn[:, hh * 80: hh * 80 + L] = V[:, :, sl] @ wo[:, sl].t()
    Ag = At * gamma.double()
    At_ln = r16((Ag - Ag.mean(-1, keepdim=True)).float())
    c2 = (At @ beta.double()).float().contiguous()                    # [B, 640]
    Bn = r16(Bn)
    # row partials of the producer: (sum, sum of squares) of every 80-column slice
    parts = 2 * ((C + 159) // 160)
    xs64 = xu.double().view(Mu, C // 80, 80)
    rs = torch.stack([xs64.sum(-1), (xs64 * xs64).sum(-1)], -1).permute(1, 0, 2).float().contiguous()     # [parts][Mu][2]
    assert rs.shape[0] == parts
    mean = x.double().mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(x.double().var(-1, unbiased=False, keepdim=True) + 1e-5)
    # (i) the kernel's formula in fp64 from the rounded operands
    S = (rstd * torch.einsum("bmc,bkc->bmk", x.double().view(B, hw, C), At_ln.double()).view(M, H * 80)
         + c2.double().repeat_interleave(hw, 0)).view(B, hw, H, 80)
    S[..., L:] = float("-inf")
    Pm = torch.softmax(S, dim=-1).view(B, hw, H * 80).float()
    ref_fold = (r.view(B, hw, C) + torch.einsum("bmk,bkc->bmc", Pm, Bn) + bo).view(M, C)
    # (ii) LayerNorm, then the unfolded attention
    xn = (((x.double() - mean) * rstd) * gamma.double() + beta.double()).float().view(B, hw, C)
    q = (xn @ wq.t()).view(B, hw, H, d).transpose(1, 2)
    kk, vv = (t.view(B, L, H, d).transpose(1, 2) for t in (K, V))
    o = F.scaled_dot_product_attention(q, kk, vv).transpose(1, 2).reshape(B, hw, C)
    ref_attn = (r.view(B, hw, C) + o @ wo.t() + bo).view(M, C)
    slot = torch.arange(H * 80)
    perm = (slot & ~12) | ((slot & 4) << 1) | ((slot & 8) >> 1)
    Bw = torch.zeros(B, C, H * 80)
    Bw[:, :, perm] = Bn.transpose(1, 2)
    At_t = At_ln.view(B, H * 80, C // 32, 32).permute(0, 2, 1, 3).contiguous()
    Bw_t = Bw.view(B, C // 32, 32, 20, 32).permute(0, 1, 3, 2, 4).contiguous()
    out = OUT((M, C))
    oparts = sdlib.sd_op_ln_partials(1, M, C)
    ors = OUT((oparts, M, 2), torch.float32)
    _lib.check(sdlib.sd_op_xattn_fused_ln(stream(), P(G(x, torch.bfloat16)), P(G(r, torch.bfloat16)), P(out), P(G(At_t, torch.bfloat16)),
                                          P(G(Bw_t, torch.bfloat16)), P(G(bo)), M, C, hw, L, P(G(rs)), parts, Mu, P(G(c2)), 1e-5, P(ors)))
    torch.cuda.synchronize()
    check_guards()
    xattn_norm2_elementwise(out, x, At_ln, c2, rs, Bn, r, bo, L, B, hw, C, Mu, f"xattn fused+norm2 B={B} hw={hw} C={C}")
    e1, e2 = rel_l2(out, ref_fold), rel_l2(out, ref_attn)
    print(f"xattn fused + norm2 B={B} hw={hw} C={C} offset={offset}: vs folded fp64 {e1:.3e}, vs LayerNorm + SDPA + linears {e2:.3e}")
    assert torch.isfinite(out.float()).all()
    assert e1 < 8e-3 and e2 < 2e-2
    tot = ors.sum(0).cpu()
    assert torch.allclose(tot[:, 0].double(), out.double().cpu().sum(1), rtol=1e-4, atol=1e-2)


@pytest.mark.parametrize("form,hw,M,pad", [
    ("v_t", 4096, 512, 64),        # V^T[C, hw] = Wv . g_img^T: M = C = 512, N = hw, ldc = hw (+ a gap here)
    ("s", 4096, 1000, 32),         # S = Q K^T from the packed q|k rows: ldx = 2C, a ragged query chunk
    ("s", 16384, 200, 32),         # ... 128 x 128 latent: N = hw = 16384
    ("pv", 4096, 1000, 64),        # O[q0 : q0 + rows] = P V + b_v: ldx = hw (+ gap), written at a row offset (coff)
    ("pv", 16384, 200, 64),
])
def test_gemm_strided_and_offset_operands_of_the_chunked_vae_attention(sdlib, form, hw, M, pad):
    """The chunked VAE mid-block attention (csrc/plan.hip, vae_attention) runs its three GEMMs on row-strided operands and
    writes at an offset into a bigger tensor.  Here every stride is wider than its rows (ldx > K1, ldx2 > K - K1, ldr > N,
    ldc > N): the gap columns are sentinel-filled and must stay so, rows of the output tensor before and after the written
    block must stay NaN, operands are read only inside their rows (NaN-poisoned gaps), and every element meets its bound."""
    C = 512
    g = torch.Generator().manual_seed(hw + M + pad)
    if form == "v_t":
        N, K, K1 = hw, C, C
        x = r16(torch.randn(M, K, generator=g) / math.sqrt(C))
        w = r16(torch.randn(N, K, generator=g))
        b = None
        ldx, ldx2 = K + pad, 0
    elif form == "s":
        N, K, K1 = hw, C, C // 2                          # the K range split over X / X2, both rows of the q|k buffer
        x = r16(torch.randn(M, K, generator=g))
        w = r16(torch.randn(N, K, generator=g) / math.sqrt(C))
        b = None
        ldx, ldx2 = 2 * C, 2 * C
    else:
        N, K, K1 = C, hw, hw
        x = r16(torch.softmax(torch.randn(M, K, generator=g) * 3, -1))
        w = r16(torch.randn(N, K, generator=g))
        b = torch.randn(N, generator=g)
        ldx, ldx2 = K + pad, 0
    res = r16(torch.randn(M, N, generator=g)) if form == "s" else None
    ldr, ldc = N + pad, N + pad
    # X (and X2) as column blocks of a row-strided buffer; poison in the gaps
    xbuf = G(torch.cat([x[:, :K1], torch.zeros(M, ldx - K1)], 1) if ldx > K1 else x[:, :K1], torch.bfloat16, ld=None)
    x1 = xbuf[:, :K1]
    x2 = None
    if K1 < K:
        x2buf = G(torch.cat([x[:, K1:], torch.zeros(M, ldx2 - (K - K1))], 1), torch.bfloat16)
        x2 = x2buf[:, :K - K1]
        for t, lo in ((xbuf, K1), (x2buf, K - K1)):
            t[:, lo:] = float("nan")
    elif ldx > K1:
        xbuf[:, K1:] = float("nan")
    rd = G(res, torch.bfloat16, ld=ldr) if res is not None else None
    row0, total = 37, M + 37 + 11                          # the output block sits at a row offset inside a bigger tensor
    outbuf = OUT((total, N), ld=ldc)
    out = outbuf[row0:row0 + M]
    _lib.check(sdlib.sd_op_gemm(stream(), P(x1), ldx, P(x2) if x2 is not None else None, ldx2, K1, P(G(w, torch.bfloat16)),
                                P(G(b)) if b is not None else None, None, P(rd) if rd is not None else None, ldr, P(out), ldc,
                                M, N, K, 0))
    torch.cuda.synchronize()
    check_guards()
    around = torch.cat([outbuf[:row0], outbuf[row0 + M:]]).view(torch.int16)
    assert (around == torch.tensor(0x7FC0, dtype=torch.int16)).all(), "rows outside the written block were stored"
    ref, bound = gemm_bound(x, w, b, None, res)
    assert rel_l2(out, ref) < TOL
    assert_elementwise(out, ref, bound, f"gemm strided {form} hw={hw} M={M}", ("row", "col"))
