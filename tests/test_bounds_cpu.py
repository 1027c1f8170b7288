"""The elementwise gate of tests/bounds.py, checked without a GPU.

Exact fp64 results rounded to the output format stand in for a correct kernel: they must pass with margin.  Faults of the
kinds the kernels risk (a halo corner, a wrapped halo column, a dropped bias, a split-K slab counted twice, a ragged key
tile, a tail row from the neighbouring image) are injected into the same results: each must pass the rel-L2 gate the GPU
tests have always used -- the gap is real -- and fail the elementwise gate.  The guard bands must catch single stray
stores and accept an untouched buffer."""
import math

import pytest
import torch
import torch.nn.functional as F

from tests.bounds import (assert_e4m3_codes, assert_elementwise, attention_ref_bound, check_guards, conv3x3_nhwc_ref,
                          elementwise_ratio, forget_guards, gemm_bound, guarded, guarded_input, linear_bound,
                          norm_ref_bound, ulp_e4m3)
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
