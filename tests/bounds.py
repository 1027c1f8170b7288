"""Per-element parity bounds and guarded device buffers for the kernel tests.

A rel-L2 gate over a whole output cannot see an error confined to a few elements (a halo corner, a tail tile, a split-K
seam).  The helpers here check every element against an a-priori bound derived from the arithmetic the kernel documents,
never fitted to observed errors:

    bound = u_out(|ref|) + c_acc * 2^-24 * K_eff * mag + atol_tiny

``ref`` is computed in float64 from the same rounded inputs the kernel reads, ``mag`` is the same operation on the absolute
values (so ``2^-24 * K_eff * mag`` is the classical worst-case bound of a length-K_eff fp32 summation in any order), and
``u_out`` is one unit in the last place of the output format at ``|ref|`` (the final rounding costs at most half of it; the
other half covers an accumulation error that crosses a binade).

``guarded`` / ``guarded_input`` place a tensor between two guard bands in one device allocation.  Output guards hold a
sentinel NaN payload that no kernel produces; input guards hold NaN (or the e4m3 NaN byte), so a read outside an operand
turns the element that used it into NaN.  ``check_guards`` asserts every guard byte, and the gap columns of a row pitch
``ld`` wider than the tensor, are still bit-identical to what was written there.
"""
import math

import torch

U32 = 2.0 ** -24            # fp32 unit roundoff
U_BF16 = 2.0 ** -9          # bf16 unit roundoff (round to nearest even)
GELU_POLY = 1.3e-5          # |gelu_hat(x) - gelu(x)| <= 1.3e-5 |x| (csrc/common.h: gelu_erf_f and geglu_pair)
ATOL_TINY = 2.0 ** -120
LN2 = math.log(2.0)

# ---------------------------------------------------------------------------------------------------------------------
# units in the last place
# ---------------------------------------------------------------------------------------------------------------------


def _ulp(a, mant_bits, min_exp=None):
    a = a.abs().double()
    _, e = torch.frexp(a)                       # a = m 2^e, m in [0.5, 1): the binade's exponent is e - 1
    e = e - 1
    if min_exp is not None:
        e = e.clamp(min=min_exp)                # subnormals share the smallest normal binade's spacing
    u = torch.ldexp(torch.ones_like(a), e - mant_bits)
    return torch.where(a > 0, u, torch.zeros_like(a)) if min_exp is None else u


def ulp_bf16(a):
    return _ulp(a, 7)


def ulp_fp32(a):
    return _ulp(a, 23)


def ulp_e4m3(a):
    """One ulp of OCP e4m3 (3 mantissa bits, smallest normal exponent -6, subnormal spacing 2^-9)."""
    return _ulp(a, 3, min_exp=-6)


ULP = {torch.bfloat16: ulp_bf16, torch.float32: ulp_fp32}

# ---------------------------------------------------------------------------------------------------------------------
# the elementwise gate
# ---------------------------------------------------------------------------------------------------------------------

def elementwise_ratio(got, ref, bound):
    got = got.detach().double().cpu()
    ref = ref.detach().double().cpu()
    bound = torch.as_tensor(bound, dtype=torch.float64).expand_as(ref)
    err = (got - ref).abs()
    err = torch.where(torch.isfinite(got), err, torch.full_like(err, float("inf")))
    return err, bound, err / bound


def assert_elementwise(got, ref, bound, what, names=None):
    """Fail if any element has |got - ref| > bound (NaN / Inf in ``got`` always fails).  ``names`` labels the index
    dimensions, e.g. ("b", "y", "x", "c").  Prints and returns the worst error / bound ratio."""
    got = got.detach()
    assert tuple(got.shape) == tuple(ref.shape), f"{what}: shape {tuple(got.shape)} vs reference {tuple(ref.shape)}"
    err, bound, ratio = elementwise_ratio(got, ref, bound)
    assert (bound > 0).all(), f"{what}: a bound is not positive"
    flat = int(torch.argmax(ratio))
    idx = tuple(int(i) for i in torch.unravel_index(torch.tensor(flat), ratio.shape))
    names = names or tuple(f"i{k}" for k in range(len(idx)))
    where = "(" + ", ".join(f"{n}={i}" for n, i in zip(names, idx)) + ")"
    worst = float(ratio.reshape(-1)[flat])
    bad = int((err > bound).sum())
    print(f"[bounds] {what}: worst err/bound {worst:.3e} at {where}")
    assert bad == 0, (f"{what}: {bad} of {err.numel()} elements exceed their bound; worst at {where}: "
                      f"got {float(got.double().cpu().reshape(-1)[flat]):.6g}, ref {float(ref.reshape(-1)[flat]):.6g}, "
                      f"err {float(err.reshape(-1)[flat]):.3e}, bound {float(bound.reshape(-1)[flat]):.3e}, "
                      f"ratio {worst:.3g}")
    return worst


def assert_e4m3_codes(got_codes, scaled_ref, acc_bound, what, names=None):
    """e4m3 outputs, compared in code units.  ``scaled_ref`` is the fp64 value the kernel rounds (already divided by the
    output scale), ``acc_bound`` the accumulation part of its bound in the same units.  The codes must be equal, except
    that one code of difference is allowed where scaled_ref lies within acc_bound of a rounding midpoint."""
    ref = scaled_ref.double().cpu().clamp(-448.0, 448.0)
    want = ref.to(torch.float8_e4m3fn)
    got = got_codes.detach().cpu().view(torch.float8_e4m3fn)
    gv, wv = got.double(), want.double()
    assert torch.isfinite(gv).all(), f"{what}: NaN code in the output"
    u = ulp_e4m3(ref)
    lo, hi = (ref.abs() / u).floor() * u, (ref.abs() / u).floor() * u + u     # the two representable neighbours
    mid_dist = (ref.abs() - 0.5 * (lo + hi)).abs()
    near_mid = mid_dist <= torch.as_tensor(acc_bound, dtype=torch.float64).expand_as(ref)
    g8, w8 = got.view(torch.uint8).to(torch.int32), want.view(torch.uint8).to(torch.int32)
    code_diff = (g8 - w8).abs()
    same_sign = (gv * wv >= 0) | (gv == 0) | (wv == 0)
    ok = (code_diff == 0) | ((gv == 0) & (wv == 0)) | (near_mid & (code_diff <= 1) & same_sign & ((gv - wv).abs() <= u * 1.0000001))
    bad = int((~ok).sum())
    err = (gv - wv).abs() / u
    flat = int(torch.argmax(err + (~ok).double() * 1e9))
    idx = tuple(int(i) for i in torch.unravel_index(torch.tensor(flat), ref.shape))
    names = names or tuple(f"i{k}" for k in range(len(idx)))
    where = "(" + ", ".join(f"{n}={i}" for n, i in zip(names, idx)) + ")"
    ndiff = int((code_diff != 0).sum())
    print(f"[bounds] {what}: {ndiff} of {ref.numel()} codes differ by one at a rounding midpoint, {bad} violations")
    assert bad == 0, (f"{what}: {bad} e4m3 codes outside the allowed difference; worst at {where}: got {float(gv.reshape(-1)[flat])}, "
                      f"want {float(wv.reshape(-1)[flat])} (fp64 {float(ref.reshape(-1)[flat]):.6g})")
    return ndiff

# ---------------------------------------------------------------------------------------------------------------------
# the flip budget: how many outputs are not the correctly rounded fp64 value
# ---------------------------------------------------------------------------------------------------------------------
# The two gates above allow every element its a-priori WORST case; for the normalisations that is the output ulp (bf16) or a
# band round every rounding midpoint that carries n_stat u (e4m3), wide enough to pass an eps 100x too large or a count off
# by one.  A kernel whose only errors are a few fp32 roundings differs from RN(fp64) on ~1e-5 .. 1e-4 of its outputs, one with
# such a mistake on 1e-3 .. 1e-1: the COUNT separates them.  The budget is never taken from the kernel: it is four times the
# count of plain fp32 restatements of the kernel's own formulas on the CPU (gn_restatements / ln_restatements), plus 8.

FLIP_FACTOR, FLIP_FLOOR, FLIP_REF_MAX = 4, 8, 1e-3


def _round_to(ref, mant_bits, min_exp=None):
    """fp64 -> the nearest value (ties to even) of a binary format with ``mant_bits`` explicit mantissa bits, in ONE rounding
    (torch converts fp64 through fp32, which rounds twice)."""
    ref = ref.double()
    u = _ulp(ref, mant_bits, min_exp)
    safe = torch.where(u > 0, u, torch.ones_like(u))
    return torch.where(u > 0, torch.round(ref / safe) * safe, torch.zeros_like(ref))


def _ordinal(codes, mag_mask):
    """Sign-magnitude codes -> integers in value order (+0 and -0 both 0): adjacent codes differ by one."""
    c = codes.to(torch.int32)
    mag = c & mag_mask
    return torch.where((c & (mag_mask + 1)) != 0, -mag, mag)


def flip_ordinals(t, kind):
    """The value-ordered code of every element of ``t`` rounded to ``kind``: "bf16" (t = a bf16 tensor, or fp32 / fp64 values
    still to be rounded) or "e4m3" (t = uint8 codes, or fp32 / fp64 values already times the output scale)."""
    t = t.detach().cpu()
    if kind == "bf16":
        if t.dtype == torch.float64:
            t = _round_to(t, 7).float()                                   # exact: the value is a bf16 number
        return _ordinal(t.to(torch.bfloat16).contiguous().view(torch.int16), 0x7fff)
    assert kind == "e4m3", kind
    if t.dtype == torch.float64:
        t = _round_to(t.clamp(-448.0, 448.0), 3, min_exp=-6).float()
    if t.dtype != torch.uint8:
        t = t.float().clamp(-448.0, 448.0).to(torch.float8_e4m3fn).view(torch.uint8)
    assert not ((t & 0x7f) == 0x7f).any(), "NaN code (0x7f)"
    return _ordinal(t, 0x7f)


def count_flips(t, ref64, kind):
    return int((flip_ordinals(t, kind) != flip_ordinals(ref64.double(), kind)).sum())


def assert_e4m3_interval(got_codes, scaled_ref, bound, what):
    """e4m3 outputs where the a-priori bound exceeds one code spacing (a GEGLU product near zero at a large output scale:
    the documented polynomial error times the scale spans several subnormal codes), so assert_e4m3_codes' "one code at a
    midpoint" cannot describe it: the code must be the rounding of SOME value within ``bound`` of scaled_ref, i.e. lie
    between RN(ref - bound) and RN(ref + bound).  Where bound is below half a code spacing this is assert_e4m3_codes' rule."""
    ref = scaled_ref.double().cpu()
    b = torch.as_tensor(bound, dtype=torch.float64).cpu().expand_as(ref)
    lo, hi, have = flip_ordinals(ref - b, "e4m3"), flip_ordinals(ref + b, "e4m3"), flip_ordinals(got_codes, "e4m3")
    bad = (have < lo) | (have > hi)
    wide = int(((hi - lo) > 1).sum())
    print(f"[bounds] {what}: {int(bad.sum())} of {ref.numel()} codes outside [RN(ref - bound), RN(ref + bound)]; the interval spans "
          f"more than two codes on {wide} elements")
    assert not bad.any(), f"{what}: {int(bad.sum())} e4m3 codes are not the rounding of any value within the bound of the fp64 value"
    return wide


def near_midpoint_count(scaled_ref, half_width):
    """How many elements of the (scaled, fp64) e4m3 reference lie within ``half_width`` of a rounding midpoint: the allowance
    of a DOCUMENTED approximation (e.g. GELU_POLY |a gate| os), computed from the reference alone."""
    ref = scaled_ref.double().cpu().clamp(-448.0, 448.0).abs()
    u = ulp_e4m3(ref)
    lo = (ref / u).floor() * u
    return int(((ref - (lo + 0.5 * u)).abs() <= torch.as_tensor(half_width, dtype=torch.float64).expand_as(ref)).sum())


def assert_flip_budget(got, ref64, restatements, kind, what, extra=0, acc_bound=None):
    """``got`` (bf16 tensor / e4m3 codes) against RN(ref64) -- for e4m3 ref64 is already times the output scale -- by COUNT:
    every element that is not the correctly rounded fp64 value must be an adjacent code, and there may be at most
    4 F_ref + 8 (+ ``extra``) of them, F_ref = the largest such count among the CPU fp32 ``restatements`` (fp32 values
    before the output rounding).  The factor 4: the kernels add v_exp_f32, v_rcp_f32 and rsqrtf at ~1 ulp each and another
    summation tree to the restatement's few fp32 roundings, and flips are proportional to the relative error; the 8 is the
    Poisson floor of counts of 0 .. 10.  F_ref <= 1e-3 numel is asserted, so the budget cannot hide a failure of the
    reference.  ``acc_bound`` (the operation's a-priori bound WITHOUT the output ulp, in ref64's units): where it reaches one
    ulp of the output format -- a bf16 output that cancels to nearly zero, whose grid is finer than fp32 noise -- a flip need
    not be to the adjacent code (it still counts, and the per-element gate still bounds it).  Prints and returns
    (flips, F_ref)."""
    want = flip_ordinals(ref64.double(), kind)
    have = flip_ordinals(got, kind)
    assert have.shape == want.shape, f"{what}: shape {tuple(have.shape)} vs reference {tuple(want.shape)}"
    numel = want.numel()
    d = (have - want).abs()
    flips = int((d != 0).sum())
    f_ref = max(int((flip_ordinals(r, kind) != want).sum()) for r in restatements)
    budget = FLIP_FACTOR * f_ref + FLIP_FLOOR + int(extra)
    print(f"[bounds] {what}: flips {flips} of {numel} (fp32 restatements F_ref {f_ref}, budget {budget}"
          + (f", of which {int(extra)} for a documented approximation" if extra else "") + ")")
    assert f_ref <= FLIP_REF_MAX * numel, f"{what}: the fp32 restatement itself flips {f_ref} of {numel} codes (> 1e-3)"
    far = d > 1
    if acc_bound is not None:
        r = ref64.double().cpu()
        u = ulp_bf16(r) if kind == "bf16" else ulp_e4m3(r.clamp(-448.0, 448.0))
        far = far & (u > torch.as_tensor(acc_bound, dtype=torch.float64).cpu().expand_as(r))
    far = int(far.sum())
    assert far == 0, f"{what}: {far} of {numel} outputs are more than one {kind} code from the rounded fp64 value"
    assert flips <= budget, (f"{what}: {flips} of {numel} outputs are not the rounded fp64 value; the fp32 restatements give "
                             f"at most {f_ref}: budget {FLIP_FACTOR} x {f_ref} + {FLIP_FLOOR}"
                             + (f" + {int(extra)}" if extra else "") + f" = {budget}")
    return flips, f_ref


def _silu32(y):
    return y / (1.0 + torch.exp(-y))                                       # fp32, as silu_f (csrc/common.h) states it


def _serial_sum(t, dim):
    """fp32 sum along ``dim`` in index order, one addition after the other."""
    acc = torch.zeros_like(t.select(dim, 0))
    for i in range(t.shape[dim]):
        acc = acc + t.select(dim, i)
    return acc


def gn_restatements(x, gamma, beta, groups, eps, silu, scale=None, cnt_add=0):
    """GroupNorm(+SiLU) of x [B, HW, C] (the kernel's bf16 input as fp32) in plain fp32, in the kernels' own formulas
    (csrc/norm.hip): one-pass variance max(E[x^2] - mean^2, 0), rstd = rsqrt(var + eps); both affine forms --
    x sc + (beta - mean sc), sc = rstd gamma (gn_apply_kernel) and (x - mean) rstd gamma + beta (gn_unit_store) -- and
    two summation orders: torch's pairwise sum over the group, and per-pixel sums added serially over the pixels.
    ``scale``: the e4m3 output scale (multiplied last, as the kernels do).  ``cnt_add`` states a wrong count (tests of the
    budget itself).  Returns the four fp32 tensors."""
    x = x.float()
    B, HW, C = x.shape
    cpg = C // groups
    xg = x.view(B, HW, groups, cpg)
    g, bt = gamma.float().view(1, 1, groups, cpg), beta.float().view(1, 1, groups, cpg)
    cnt = torch.tensor(float(HW * cpg + cnt_add), dtype=torch.float32)
    eps = torch.tensor(eps, dtype=torch.float32)
    flat = xg.permute(0, 2, 1, 3).reshape(B, groups, HW * cpg)
    sums = [(flat.sum(-1), (flat * flat).sum(-1)),
            (_serial_sum(xg.sum(3), 1), _serial_sum((xg * xg).sum(3), 1))]
    out = []
    for s, q in sums:
        mean = (s / cnt).view(B, 1, groups, 1)
        var = ((q / cnt).view(B, 1, groups, 1) - mean * mean).clamp(min=0.0)
        rstd = torch.rsqrt(var + eps)
        sc = rstd * g
        for y in (xg * sc + (bt - mean * sc), (xg - mean) * rstd * g + bt):
            if silu:
                y = _silu32(y)
            if scale is not None:
                y = y * scale
            out.append(y.reshape(B, HW, C))
    return out


def ln_restatements(x, gamma, beta, eps, scale=None):
    """LayerNorm of x [rows, C] in plain fp32 as layernorm_kernel / layernorm_grouped_kernel state it (csrc/norm.hip):
    two passes -- mean, then sum((x - mean)^2) -- rstd = rsqrt(q / C + eps), (x - mean) rstd gamma + beta; torch's pairwise
    row sums and serial ones."""
    x = x.float()
    C = x.shape[-1]
    eps = torch.tensor(eps, dtype=torch.float32)
    out = []
    for total in (lambda t: t.sum(-1, keepdim=True), lambda t: _serial_sum(t, 1).unsqueeze(-1)):
        mean = total(x) / C
        d = x - mean
        rstd = torch.rsqrt(total(d * d) / C + eps)
        y = d * rstd * gamma.float() + beta.float()
        out.append(y * scale if scale is not None else y)
    return out

# ---------------------------------------------------------------------------------------------------------------------
# bounds per operation
# ---------------------------------------------------------------------------------------------------------------------


def linear_bound(ref, mag, k_eff, out=torch.bfloat16, c_acc=1.0):
    """GEMM / conv / GEMV with fp32 accumulation of exact bf16 x bf16 products: one output ulp (rounding) + the
    worst-case fp32 summation error of k_eff terms (k_eff counts the epilogue's bias / bias2 / residual additions).
    The summation term is the worst case for ANY order: the MFMA's internal accumulation order is not documented, so no
    smaller a-priori bound holds.  For bf16 outputs the ulp term dominates (worst ratios ~0.5); for fp32 outputs
    (conv_out, the time-embedding GEMVs) the summation term dominates and observed ratios sit near 1e-3."""
    return ULP[out](ref) + c_acc * U32 * k_eff * mag + ATOL_TINY


def gemm_ref(x, w, bias=None, bias2=None, res=None):
    """fp64 X W^T (+ bias + bias2 + R) and its magnitude |X| |W|^T + |bias| + |bias2| + |R|."""
    x, w = x.double(), w.double()
    ref, mag = x @ w.t(), x.abs() @ w.abs().t()
    for t in (bias, bias2, res):
        if t is not None:
            ref, mag = ref + t.double(), mag + t.double().abs()
    return ref, mag


def gemm_bound(x, w, bias=None, bias2=None, res=None, out=torch.bfloat16):
    ref, mag = gemm_ref(x, w, bias, bias2, res)
    return ref, linear_bound(ref, mag, x.shape[-1] + 3, out)


def geglu_ref_bound(a, da, gate, dg, out_ulp=True):
    """value * GELU(gate) from fp64 (value, gate) and absolute error bounds (da, dg) of the kernel's fp32 factors: carried
    through the product (|d gelu / dx| <= 1.13), plus the epilogue's documented polynomial error (GELU_POLY |x|) and a few
    fp32 roundings of its own products; then the bf16 output ulp."""
    a, gate = a.double(), gate.double()
    ge = gate * 0.5 * (1.0 + torch.erf(gate / math.sqrt(2.0)))
    ref = a * ge
    acc = da * ge.abs() + 1.13 * (a.abs() + da) * dg
    rounding = ULP[torch.bfloat16](ref) if out_ulp else 0.0          # out_ulp=False: the caller rounds (e4m3 codes)
    return ref, rounding + acc + GELU_POLY * (a * gate).abs() + 8 * U32 * ref.abs() + ATOL_TINY


def fp8_gemm_ref_bound(xq, xs, wq, wsc, bias=None, res=None):
    """The fp8 GEMM from e4m3 values: (xq . wq^T) wsc / xs (+ bias + R).  The products of e4m3 values are exact in fp32; the
    epilogue multiplies by wscale[n] and 1 / xscale (two more fp32 roundings, counted with the bias / residual adds)."""
    acc, mag = xq.double() @ wq.double().t(), xq.double().abs() @ wq.double().abs().t()
    f = wsc.double() / xs
    ref, mag = acc * f, mag * f
    for t in (bias, res):
        if t is not None:
            ref, mag = ref + t.double(), mag + t.double().abs()
    return ref, mag, xq.shape[-1] + 6


def fp8_conv_ref(xin, wq, wsc, bias=None, bias2=None, res=None, stride=1, up=0):
    """The fp8 3x3 conv from e4m3 values (xin = the dequantised NCHW activations, wq the weight codes' values), NHWC, with its
    magnitude and the accumulation length (9 Cin products, the scale multiplies and the epilogue adds)."""
    ref, mag = conv3x3_nhwc_ref(xin, wq, None, None, None, stride, up)
    f = wsc.double()
    ref, mag = ref * f, mag * f
    for t in (bias, bias2):
        if t is not None:
            ref, mag = ref + t.double(), mag + t.double().abs()
    if res is not None:
        rr = res.double().permute(0, 2, 3, 1)
        ref, mag = ref + rr, mag + rr.abs()
    return ref, mag, 9 * xin.shape[1] + 6


def ln_fold_ref_bound(h, wg, c1, c2, s, q, eps):
    """The LayerNorm-folded GEMM z = rstd (h . wg - mean c1) + c2 from the kernel's operands (h [M, C] bf16 rows, wg the
    gamma-scaled bf16 weight, c1 / c2 fp32 vectors, s / q the rows' (sum, sum of squares) in fp64 from the fp32 partials
    the kernel reads).  Returns (z, dz): dz = the fp32 accumulation of h . wg and of mean c1, the fp32 E[x^2] - mean^2
    (4 u E[x^2] plus the partials' combination) through rsqrt, and the final multiply-add."""
    C = h.shape[-1]
    hd, w = h.double(), wg.double()
    mean, ex2 = s.double().view(-1, 1) / C, q.double().view(-1, 1) / C
    var = (ex2 - mean * mean).clamp(min=0.0)
    rstd = 1.0 / torch.sqrt(var + eps)
    drel = (8 + 16) * U32 * ex2 / (2 * (var + eps)) + 2 * U32
    dot = hd @ w.t() - mean * c1.double()
    mag = hd.abs() @ w.abs().t() + mean.abs() * c1.double().abs()
    z = rstd * dot + c2.double()
    dz = rstd * U32 * (C + 4) * mag + drel * (rstd * dot).abs() + 4 * U32 * (z.abs() + c2.double().abs())
    return z, dz


def subpixel_ref(x, w4p, bias):
    """Upsample2D as four 2x2 convs on the low-res NCHW input, from the packed bf16 phase weights the kernel reads
    ([4 phases][Cout][Cin/64][4 taps][64]); NHWC fp64 output and its magnitude."""
    import torch.nn.functional as F
    B, Cin, H, W = x.shape
    Cout = w4p.shape[1]
    w4 = w4p.double().permute(0, 1, 3, 2, 4).reshape(4, Cout, 2, 2, Cin).permute(0, 1, 4, 2, 3)
    xd = x.double()
    ref = torch.empty(B, Cout, 2 * H, 2 * W, dtype=torch.float64)
    mag = torch.empty_like(ref)
    for py in (0, 1):
        for px in (0, 1):
            wp = w4[2 * py + px]
            ref[:, :, py::2, px::2] = F.conv2d(xd, wp, padding=1)[:, :, py:py + H, px:px + W]
            mag[:, :, py::2, px::2] = F.conv2d(xd.abs(), wp.abs(), padding=1)[:, :, py:py + H, px:px + W]
    b = bias.double()[None, :, None, None]
    return (ref + b).permute(0, 2, 3, 1), (mag + b.abs()).permute(0, 2, 3, 1)


def conv3x3_nhwc_ref(x, w, bias=None, bias2=None, res=None, stride=1, up=0):
    """fp64 3x3 conv (pad 1) on NCHW inputs, returned NHWC with its magnitude; up = nearest 2x first."""
    import torch.nn.functional as F
    x, w = x.double(), w.double()
    if up:
        x = F.interpolate(x, scale_factor=2.0, mode="nearest")
    ref = F.conv2d(x, w, None, stride=stride, padding=1)
    mag = F.conv2d(x.abs(), w.abs(), None, stride=stride, padding=1)
    for t in (bias, bias2):
        if t is not None:
            ref, mag = ref + t.double()[None, :, None, None], mag + t.double().abs()[None, :, None, None]
    if res is not None:
        ref, mag = ref + res.double(), mag + res.double().abs()
    return ref.permute(0, 2, 3, 1), mag.permute(0, 2, 3, 1)


def norm_ref_bound(x, gamma, beta, n_stat, eps, silu, groups=None, stats=None, out_ulp=True):
    """GroupNorm (groups given, x [B, HW, C]) or LayerNorm (x [rows, C]) in fp64 from the kernel's input ``x``.

    The kernel sums x and x^2 over n_stat elements in fp32 and forms var = E[x^2] - mean^2:
      d mean <= n_stat u E|x|;  d var <= n_stat u E[x^2] + 2 |mean| d mean + 2 u E[x^2];
      d rstd / rstd <= d var / (2 (var + eps)) + 2 u (rsqrt);
    carried into |gamma| rstd (d mean + |x - mean| d rstd / rstd), a few fp32 roundings of the affine step, |silu'| <= 1.1
    and a few ulp of SiLU's exp2 / rcp; then the bf16 output ulp.
    ``stats`` = (sum, sum of squares) in fp64 from the kernel's own fp32 partials: the statistics term then only
    carries the few fp32 additions that combine them (n_stat = the number of partials)."""
    xd = x.double()
    g, bt = gamma.double(), beta.double()
    if groups is not None:
        B, HW, C = xd.shape
        xg = xd.view(B, HW, groups, C // groups)
        if stats is None:
            mean = xg.mean((1, 3), keepdim=True)
            ex2 = (xg * xg).mean((1, 3), keepdim=True)
        else:
            s, q = stats
            cnt = HW * (C // groups)
            mean, ex2 = (s / cnt).view(B, 1, groups, 1), (q / cnt).view(B, 1, groups, 1)
        eabs = xg.abs().mean((1, 3), keepdim=True)
        var = (ex2 - mean * mean).clamp(min=0.0)
        rstd = 1.0 / torch.sqrt(var + eps)
        xm = xg - mean
        shape = (1, 1, groups, C // groups)
        gg, bb = g.view(shape), bt.view(shape)
    else:
        if stats is None:
            mean = xd.mean(-1, keepdim=True)
            ex2 = (xd * xd).mean(-1, keepdim=True)
        else:
            s, q = stats
            mean, ex2 = s.view(-1, 1) / xd.shape[-1], q.view(-1, 1) / xd.shape[-1]
        eabs = xd.abs().mean(-1, keepdim=True)
        var = (ex2 - mean * mean).clamp(min=0.0)
        rstd = 1.0 / torch.sqrt(var + eps)
        xm = xd - mean
        gg, bb = g, bt
    dmean = n_stat * U32 * eabs
    dvar = n_stat * U32 * ex2 + 2 * mean.abs() * dmean + 2 * U32 * ex2
    drel = dvar / (2 * (var + eps)) + 2 * U32
    y = xm * rstd * gg + bb
    dy = gg.abs() * rstd * (dmean + xm.abs() * drel) + 4 * U32 * ((xm * rstd * gg).abs() + bb.abs())
    if silu:
        sig = torch.sigmoid(y)
        ref = y * sig
        dy = 1.1 * dy + 4 * U32 * ref.abs()
    else:
        ref = y
    ref, dy = ref.reshape(x.shape), dy.reshape(x.shape)
    return ref, (ULP[torch.bfloat16](ref) if out_ulp else 0.0) + dy + ATOL_TINY


def round_bf16_f32(t):
    """Round to bf16 (round to nearest even) a value the kernel holds in fp32."""
    return t.float().to(torch.bfloat16).double()


def attention_ref_bound(q, k, v, scale, q_rounded=False, causal=False, chunk=1):
    """Flash attention per element, q / k / v [B, heads, N, D] (bf16-rounded values).

    Reference in fp64: o = softmax(c q . k) v in exp2 units, c = scale log2 e.  Where the kernel rounds Q c to bf16 before
    QK^T (attention.hip, attn_pipe40_kernel: Q <- bf16(Q * scale * log2 e)) the reference uses that rounded Q.
    Bound: bf16 ulp of o
      + 2^-9 (P|V| + |o|): P is rounded to bf16 before PV (numerator and, if it sums rounded values, the normaliser)
      + ln2 d_s (P|V| + |o|) 2: fp32 scores carry <= (D + 1) u (|q||k| + |M|) (the +1: the pipelined kernel's stale
        reference M rides in the product as one more column), <= 2 (D + 1) u ||q|| max ||k|| (Cauchy-Schwarz)
      + u (Nk + 4 tiles + 16) P|V|: PV accumulation, per-tile rescales, exp2 / rcp ulps."""
    B, H, Nq, D = q.shape
    Nk = k.shape[2]
    c = scale * 1.4426950408889634
    qd = round_bf16_f32(q.float() * c) if q_rounded else q.double() * c
    kd, vd = k.double(), v.double()
    ref = torch.empty(B, H, Nq, D, dtype=torch.float64)
    bound = torch.empty_like(ref)
    kn = kd.norm(dim=-1).amax(-1)                                           # [B, H]
    for b in range(B):
        for h in range(H):
            s = qd[b, h] @ kd[b, h].t()                                     # [Nq, Nk], log2 units
            if causal:
                s = s.masked_fill(torch.ones(Nq, Nk, dtype=torch.bool).triu(1), float("-inf"))
            p = torch.exp2(s - s.amax(-1, keepdim=True))
            l = p.sum(-1, keepdim=True)
            o = (p @ vd[b, h]) / l
            pv = (p @ vd[b, h].abs()) / l
            ds = 2 * (D + 1) * U32 * qd[b, h].norm(dim=-1, keepdim=True) * kn[b, h]
            ntile = (Nk + 63) // 64
            bd = (ULP[torch.bfloat16](o) + U_BF16 * (pv + o.abs()) + 2 * LN2 * ds * (pv + o.abs())
                  + U32 * (Nk + 4 * ntile + 16) * pv + ATOL_TINY)
            ref[b, h], bound[b, h] = o, bd
    return ref, bound


def softmax_rows_ref_bound(s, ds, scale=1.0):
    """Row softmax of fp64 scores s with a per-element score error bound ds (score units), output rounded to bf16:
    |d p_j| <= p_j (2^{log2e scale (ds_j + max ds)} - 1) and a few fp32 ulps of exp2 / sum / rcp."""
    c = scale * 1.4426950408889634
    sm = s * c
    p = torch.exp2(sm - sm.amax(-1, keepdim=True))
    p = p / p.sum(-1, keepdim=True)
    dmax = ds.amax(-1, keepdim=True)
    dp = p * (torch.exp2(c * (ds + dmax)) - 1.0) + (s.shape[-1] + 8) * U32 * p
    return p, ULP[torch.bfloat16](p) + dp + ATOL_TINY

# ---------------------------------------------------------------------------------------------------------------------
# guarded device buffers
# ---------------------------------------------------------------------------------------------------------------------

GUARD_ROWS = 256            # the largest kernel tile, in rows
GUARD_MIN_BYTES = 64 << 10

_INT = {1: torch.uint8, 2: torch.int16, 4: torch.int32}
# output guards: NaN payloads no kernel writes (bf16 0x7FA5, fp32 0x7FA5A5A5) and a fixed byte for 8-bit outputs
SENTINEL = {2: 0x7FA5, 4: 0x7FA5A5A5, 1: 0xA5}
# input guards: plain NaN (bf16 0x7FC0, fp32 0x7FC00000) and the e4m3 NaN byte 0x7F
POISON = {2: 0x7FC0, 4: 0x7FC00000, 1: 0x7F}

_LIVE = []


class _Guard:
    def __init__(self, buf, front, rows, ld, width, pattern, label):
        self.buf, self.front, self.rows, self.ld, self.width, self.pattern, self.label = buf, front, rows, ld, width, pattern, label

    def violations(self):
        bits = self.buf.view(_INT[self.buf.element_size()])
        n = self.rows * self.ld
        pat = torch.tensor(self.pattern, dtype=torch.int64).to(bits.dtype).item()
        out = []
        front = bits[:self.front]
        bad = torch.nonzero(front != pat).flatten()
        if bad.numel():
            i = int(bad[-1])
            out.append(f"{bad.numel()} front-guard elements written, the last {self.front - i} element(s) before the start")
        back = bits[self.front + n:]
        bad = torch.nonzero(back != pat).flatten()
        if bad.numel():
            i = int(bad[0])
            out.append(f"{bad.numel()} back-guard elements written, the first {i} element(s) past the end "
                       f"(row {self.rows + i // self.ld} of a {self.rows}-row tensor)")
        if self.ld > self.width:
            gap = bits[self.front:self.front + n].view(self.rows, self.ld)[:, self.width:]
            bad = torch.nonzero(gap != pat)
            if bad.numel():
                r, cc = (int(t) for t in bad[0])
                out.append(f"{bad.shape[0]} ld-gap elements written, the first at row {r}, column {self.width + cc}")
        return out


def _make(shape, dtype, ld, guard_rows, pattern, label, device):
    shape = tuple(int(s) for s in shape)
    width = shape[-1] if shape else 1
    rows = math.prod(shape[:-1]) if len(shape) > 1 else 1
    ld = width if ld is None else int(ld)
    assert ld >= width, "ld smaller than the row width"
    es = torch.empty((), dtype=dtype).element_size()
    front = max(guard_rows * ld, -(-GUARD_MIN_BYTES // es))
    front = -(-front // (256 // es)) * (256 // es)                   # keep the tensor 256-byte aligned
    buf = torch.empty(2 * front + rows * ld, dtype=dtype, device=device)
    buf.view(_INT[es]).fill_(torch.tensor(pattern, dtype=torch.int64).to(_INT[es]).item())
    t = buf[front:front + rows * ld].view(*(shape[:-1] or (1,)), ld)[..., :width]
    if not shape:
        t = t.reshape(())
    elif len(shape) == 1:
        t = t.reshape(width)
    g = _Guard(buf, front, rows, ld, width, pattern, label)
    _LIVE.append(g)
    return t


def guarded(shape, dtype, guard_rows=GUARD_ROWS, ld=None, fill=float("nan"), label="output", device="cuda"):
    """An output tensor of ``shape`` (rows of the last dimension, row pitch ``ld`` elements) between two sentinel guards
    of >= guard_rows rows and >= 64 KiB each; the tensor itself is pre-filled with ``fill`` (NaN: an element the kernel
    never writes stays NaN).  Gap columns of an ld > width row hold the sentinel too."""
    es = torch.empty((), dtype=dtype).element_size()
    t = _make(shape, dtype, ld, guard_rows, SENTINEL[es], label, device)
    if fill is not None:
        if dtype in (torch.uint8, torch.float8_e4m3fn):
            t.view(torch.uint8).fill_(0xFF if fill != fill else int(fill))
        else:
            t.fill_(fill)
    return t


def guarded_input(src, dtype=None, guard_rows=GUARD_ROWS, ld=None, label="input", device="cuda"):
    """A device copy of ``src`` (cast to ``dtype``) between two NaN-poisoned guards; ld > width fills the gap columns
    with the same poison.  An output element that depends on memory outside its operand becomes NaN."""
    dtype = dtype or src.dtype
    es = torch.empty((), dtype=dtype).element_size()
    t = _make(src.shape, dtype, ld, guard_rows, POISON[es], label, device)
    if dtype == torch.float8_e4m3fn and src.dtype == torch.uint8:
        t.view(torch.uint8).copy_(src.to(t.device))
    else:
        t.copy_(src.to(t.device, dtype))
    return t


def is_guarded(t):
    """True if ``t`` lives in a buffer made by guarded() / guarded_input() since the last check_guards()."""
    if not isinstance(t, torch.Tensor) or t.device.type == "cpu":
        return False
    base = t.untyped_storage().data_ptr()
    return any(g.buf.untyped_storage().data_ptr() == base for g in _LIVE)


def device_operand(t, dtype=None):
    """The tensor a kernel is handed: a guarded buffer as it is, anything else copied into a guarded input."""
    if is_guarded(t) and (dtype is None or t.dtype == dtype):
        return t
    return guarded_input(t, dtype)


def check_guards():
    """Assert every guard (and ld gap) of every buffer made since the last call is untouched; then forget them."""
    n_in = sum(g.pattern == POISON[g.buf.element_size()] for g in _LIVE)
    if _LIVE:
        print(f"[guards] {len(_LIVE) - n_in} outputs, {n_in} inputs")
    try:
        for g in _LIVE:
            v = g.violations()
            assert not v, f"guard of {g.label} {tuple([g.rows, g.width])} (ld {g.ld}) overwritten: " + "; ".join(v)
    finally:
        _LIVE.clear()


def forget_guards():
    _LIVE.clear()

# ---------------------------------------------------------------------------------------------------------------------
# per-family checks shared by the kernel test files
# ---------------------------------------------------------------------------------------------------------------------

NHWC = ("b", "y", "x", "c")


def pipe40(D, Nk):
    """attn_pipe40_kernel takes d = 40 with a multiple-of-64 key count >= 256; it rounds Q * scale * log2 e to bf16."""
    return D == 40 and Nk % 64 == 0 and Nk >= 256


def heads_view(t, B, N, heads, D):
    """[B, N, heads * D] -> [B, heads, N, D], as the bf16 values the kernel reads."""
    return t.to(torch.bfloat16).float().cpu().view(B, N, heads, D).permute(0, 2, 1, 3)


def conv_gn_elementwise(x, w, b, b2, r, gamma, beta, y, normed, what, flip=()):
    """The conv output against its fp64 reference; each normalised output chained from the kernel's own stored conv output
    (statistics of the bf16-rounded values, as the epilogue sums them).  ``flip``: the indices of ``normed`` that come from
    the GroupNorm kernels' own statistics and also get the flip budget."""
    B, Cout, H, W = x.shape[0], w.shape[0], x.shape[-2], x.shape[-1]
    r64, m64 = conv3x3_nhwc_ref(x, w, b, b2, r)
    assert_elementwise(y, r64, linear_bound(r64, m64, 9 * x.shape[1] + 3), what + " conv", NHWC)
    yk = y.float().cpu().view(B, H * W, Cout)
    n64, nb = norm_ref_bound(yk, gamma, beta, H * W * Cout // 32, 1e-5, True, groups=32)
    for i, t in enumerate(normed):
        assert_elementwise(t.view(B, H * W, Cout), n64, nb, what + f" groupnorm[{i}]", ("b", "pixel", "c"))
        if i in flip:
            assert_flip_budget(t.view(B, H * W, Cout), n64, gn_restatements(yk, gamma, beta, 32, 1e-5, True), "bf16",
                               what + f" groupnorm[{i}]", acc_bound=nb - ulp_bf16(n64))


def ln_fold_elementwise(out, h, wg, c1, c2, rs, epi, what, rows=None, idx=None):
    """The LayerNorm-folded GEMM per element from the kernel's operands: the rows h, the (sum, sum of squares) partials rs
    [parts][M][2] it reads, the gamma-scaled weight and c1 / c2.  rows: a row subset to check (big bench shapes); idx: the
    GEGLU packing (weight row q is the natural column idx[q])."""
    tot = rs.double().cpu().sum(0)
    hh, oo = h.to(torch.bfloat16).float().cpu(), out
    if rows is not None:
        hh, tot, oo = hh[rows], tot[rows], out[rows]
    z, dz = ln_fold_ref_bound(hh, wg.float().cpu(), c1.float().cpu(), c2.float().cpu(), tot[:, 0], tot[:, 1], 1e-5)
    if idx is not None:
        inv = torch.argsort(idx)
        z, dz = z[:, inv], dz[:, inv]
    if epi:
        H = z.shape[1] // 2
        ref, bound = geglu_ref_bound(z[:, :H], dz[:, :H], z[:, H:], dz[:, H:])
    else:
        ref, bound = z, ulp_bf16(z) + dz + ATOL_TINY
    assert_elementwise(oo, ref, bound, what, ("row", "col"))


def attention_elementwise(out, q, k, v, heads, D, what, causal=False):
    """Per element against attention_ref_bound, q / k / v / out [B, N, heads * D].  Above 2^29 scores the fp64 reference
    covers the first and last head of every sample (each head is its own work item; guards and rel-L2 cover the rest)."""
    B, Nq, Nk = q.shape[0], q.shape[1], k.shape[1]
    hs = list(range(heads)) if B * heads * Nq * Nk <= 2 ** 29 else [0, heads - 1]
    qh, kh, vh, oh = (heads_view(t, B, n, heads, D)[:, hs] for t, n in ((q, Nq), (k, Nk), (v, Nk), (out, Nq)))
    ref, bound = attention_ref_bound(qh, kh, vh, 1.0 / math.sqrt(D), q_rounded=pipe40(D, Nk), causal=causal)
    assert_elementwise(oh, ref, bound, what, ("b", "head", "row", "d"))


def grouped_softmax_elementwise(out, s, ds, L, what):
    """softmax over the first L of every 80 columns from fp64 scores s with per-element error bounds ds; the other columns
    are exactly 0."""
    M, N = s.shape
    sg, dg = s.view(M, N // 80, 80), ds.view(M, N // 80, 80)
    p, pb = softmax_rows_ref_bound(sg[..., :L], dg[..., :L])
    ref = torch.zeros(M, N // 80, 80, dtype=torch.float64)
    bound = torch.full_like(ref, ATOL_TINY)
    ref[..., :L], bound[..., :L] = p, pb
    assert_elementwise(out.view(M, N // 80, 80), ref, bound, what, ("row", "head", "slot"))


def xattn_elementwise(out, S, Smag, s_rel, Bn, r, bo, L, what, S_abs_err=None):
    """Y = R + sum_h softmax_L(S_h) B_h + b per element, S [B, hw, 640] fp64 scores of the kernel's own operands.
    Score error: s_rel * Smag (fp32 accumulation; plus S_abs_err where the scores carry a normalisation); through softmax
    |d p_j| <= p_j (e^{ds_j + max ds} - 1); the probabilities are rounded to bf16 before the second product (2^-9, numerator
    and normaliser); fp32 accumulation of the second product, residual and bias; bf16 output."""
    B, hw, N = S.shape
    H = N // 80
    ds = s_rel * Smag + (S_abs_err if S_abs_err is not None else 0.0)
    Sg, dg = S.view(B, hw, H, 80)[..., :L], ds.view(B, hw, H, 80)[..., :L]
    p = torch.softmax(Sg, -1)
    pe = p * (torch.exp(dg + dg.amax(-1, keepdim=True)) - 1.0) + 2 * 2.0 ** -9 * p + (L + 8) * U32 * p
    full = lambda t: torch.cat([t, torch.zeros(B, hw, H, 80 - L, dtype=t.dtype)], -1).view(B, hw, N)
    Bd = Bn.double()
    y = torch.einsum("bmk,bkc->bmc", full(p), Bd) + r.double().view(B, hw, -1) + bo.double()
    pa = torch.einsum("bmk,bkc->bmc", full(p), Bd.abs())
    bound = (ulp_bf16(y) + torch.einsum("bmk,bkc->bmc", full(pe), Bd.abs())
             + U32 * (N + 3) * (pa + r.double().abs().view(B, hw, -1) + bo.double().abs()) + ATOL_TINY)
    assert_elementwise(out.view(B, hw, -1), y, bound, what, ("b", "row", "c"))


def sample_rows(B, hw):
    """Samples 0 and B - 1 (and one between when B > 2): the fp64 reference of every row of the largest cases would
    dominate the suite's time."""
    return sorted({0, B // 2, B - 1})


def softmax_rows_elementwise(out, s, scale, what):
    """The VAE's row softmax of bf16 scores s: exp2((s - max) scale log2 e) in fp32 -- the argument carries a few ulp of
    (|s| + |max|) scale log2 e -- then the row sum, the reciprocal and the bf16 output."""
    sd = s.double()
    ds = 4 * U32 * (sd.abs() + sd.abs().amax(-1, keepdim=True))
    p, pb = softmax_rows_ref_bound(sd, ds, scale)
    assert_elementwise(out, p, pb, what, ("row", "col"))


def xattn_norm2_elementwise(out, x, At_ln, c2, rs, Bn, r, bo, L, B, hw, C, Mu, what):
    """The fused cross-attention with norm2 folded in, per element on sample_rows(): scores rstd (x . A_ln) + c2 from the
    kernel's operands, rstd from the (sum, sum of squares) partials rs [parts][Mu][2] it reads (row m uses m % Mu); the
    score error adds the fp32 E[x^2] - mean^2 through rsqrt and the final multiply-add to the accumulation term."""
    M = B * hw
    sel = sample_rows(B, hw)
    tot = rs.double().cpu().sum(0).repeat(M // Mu, 1).view(B, hw, 2)[sel]
    x64, A64 = x.double().cpu().view(B, hw, C)[sel], At_ln.double().cpu()[sel]
    ex2, mu = tot[..., 1:] / C, tot[..., :1] / C
    var = (ex2 - mu * mu).clamp(min=0.0)
    rstd = 1.0 / torch.sqrt(var + 1e-5)
    drel = 24 * U32 * ex2 / (2 * (var + 1e-5)) + 2 * U32
    dot = torch.einsum("bmc,bkc->bmk", x64, A64)
    c2s = c2.double().cpu()[sel][:, None, :]
    S = rstd * dot + c2s
    S_err = drel * (rstd * dot).abs() + 4 * U32 * (S.abs() + c2s.abs())
    xattn_elementwise(out.view(B, hw, C)[sel], S, rstd * torch.einsum("bmc,bkc->bmk", x64.abs(), A64.abs()), U32 * (C + 2),
                      Bn[sel], r.view(B, hw, C)[sel], bo, L, what, S_abs_err=S_err)
