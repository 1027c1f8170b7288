"""Self-attention guidance on the GPU: the two kernels of csrc/sag.hip and the SAG forms of the step kernels per element against
fp64 restatements (guard bands round every buffer), the UNet's mass capture against the SAG oracle (tests/sag_oracle.py), one
full SAG step, and the pipeline against the oracle loop.

Tolerances (tests/bounds.py's rule for an fp32 output: one ulp plus 2^-24 K mag, K the longest input-to-output path).
* The mass.  A logit is a D-term fp32 sum of exact bf16 products: |ds| <= D 2^-24 A, A = the largest sum_i |q_i k_i| of the
  case.  A probability's relative error is that of its exponential and of its row sum: 2 D A (numerator and denominator), the
  subtraction of the max and the exponential itself (4), the N-term row sum, the reciprocal and the product (N + 2).  A mass is
  a sum of N heads positive probabilities (N heads) and one scaling (2):  K = 2 D A + 2 N + N heads + 8, mag = the mass.  The
  issue's estimate is 2e-4 relative; the derived figure is asserted at or below 1e-3 for every case.
* The degrade pass: coefficient, product and fma of x0 (3), weight rounding and nine fmas per blur pass (2 x 10), coefficient,
  product and fma of the output (3): K = 26 on the propagated magnitudes.
* The step kernels: tests/test_pag_gpu.py's counts (the SAG term has the PAG term's three operations).
* The UNet and the pipeline: UNET_TOL of tests/test_unet_gpu.py and FREE_TOL / FREE_COS of tests/test_pipeline_gpu.py; the masks
  outside the band tests/sag_oracle.py derives from the oracle alone."""
import ctypes as C
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from sonicdiffusionbayeslab_amd import _lib
from tests import bounds as BD
from tests import sag_oracle as so
from tests.util import cosine, oracle_cfg, rel_l2

UNET_TOL = so.UNET_TOL
FREE_TOL, FREE_COS = so.FREE_TOL, so.FREE_COS
GUIDE_CFG_SAG, GUIDE_SAG = 4, 5     # include/sd_hip.h
GS, SAG = so.GS, so.SAG_SCALE
K_STEP, K_PC = 13, 15               # tests/test_pag_gpu.py
K_DEGRADE = 26
U = 2.0 ** -24


@pytest.fixture(autouse=True)
def _drop_guards():
    yield
    torch.cuda.synchronize()
    BD.forget_guards()


def stream():
    return torch.cuda.current_stream().cuda_stream


def bits32(t):
    return t.contiguous().view(torch.int32)


def f32(v):
    return float(torch.tensor(v, dtype=torch.float32))


# ------------------------------------------------------------------------------------------------------ 1. the mass op
#              B  heads  N    D    extra pitch  exp2 units
MASS_CASES = [(2, 8, 16, 160, 0, 0), (2, 8, 20, 160, 0, 0), (1, 8, 63, 160, 0, 0), (1, 20, 144, 64, 0, 0), (2, 8, 256, 80, 0, 0),
              (3, 8, 256, 160, 0, 0), (2, 8, 20, 160, 64, 0), (1, 8, 63, 160, 0, 1), (2, 8, 256, 80, 0, 1)]


def _mass_inputs(B, heads, N, D, exp2):
    """bf16 Q | K | V rows whose logits have standard deviation about 1.5 (Q carries the scale: nothing else is applied)."""
    g = torch.Generator().manual_seed(B * 1000 + heads * 100 + N + D)
    Cc = heads * D
    amp = math.sqrt(1.5 / math.sqrt(D))
    qkv = torch.randn(B * N, 3 * Cc, generator=g)
    qkv[:, :2 * Cc] *= amp
    if exp2:
        qkv[:, :Cc] *= math.log2(math.e)
    return qkv.to(torch.bfloat16)


def _mass_ref_bound(qkv, B, heads, N, D, exp2):
    Cc = heads * D
    q = qkv[:, :Cc].double().view(B, N, Cc)
    k = qkv[:, Cc:2 * Cc].double().view(B, N, Cc)
    ref = so.attn_mass(q, k, heads, scale=math.log(2.0) if exp2 else 1.0)
    qa, ka = q.abs().view(B, N, heads, D).transpose(1, 2), k.abs().view(B, N, heads, D).transpose(1, 2)
    A = float((qa @ ka.transpose(-1, -2)).max()) * (math.log(2.0) if exp2 else 1.0)
    K = 2 * D * A + 2 * N + N * heads + 8
    return ref, K


def _launch_mass(sdlib, qkv, B, heads, N, D, extra, exp2):
    Cc = heads * D
    ld = 3 * Cc + extra
    src = BD.guarded_input(qkv, torch.bfloat16, ld=ld, label="qkv")
    out = BD.guarded((B, N), torch.float32, label="mass")
    _lib.check(sdlib.sd_op_sag_attn_mass(stream(), src.data_ptr(), src.data_ptr() + 2 * Cc, ld, out.data_ptr(), B, heads, N, D, exp2),
               "sd_op_sag_attn_mass")
    torch.cuda.synchronize()
    got = out.cpu().clone()
    BD.check_guards()
    return got


@pytest.mark.parametrize("B,heads,N,D,extra,exp2", MASS_CASES,
                         ids=[f"B{c[0]}-h{c[1]}-N{c[2]}-d{c[3]}" + ("-wide" if c[4] else "") + ("-exp2" if c[5] else "") for c in MASS_CASES])
def test_attn_mass_per_element(sdlib, B, heads, N, D, extra, exp2):
    assert sdlib.sd_sag_mass_check(B, heads, N, D, 3 * heads * D + extra, 0) == 0
    qkv = _mass_inputs(B, heads, N, D, exp2)
    ref, K = _mass_ref_bound(qkv, B, heads, N, D, exp2)
    tol = K * U
    print(f"[sag mass] B{B} h{heads} N{N} d{D}: K = {K:.0f}, relative tolerance {tol:.2e}; mass std {float(ref.std()):.3f} "
          f"range {float(ref.min()):.2f} .. {float(ref.max()):.2f}")
    assert tol <= 1e-3
    got = _launch_mass(sdlib, qkv, B, heads, N, D, extra, exp2)
    bound = BD.linear_bound(ref, ref.abs(), K, out=torch.float32)
    BD.assert_elementwise(got, ref, bound, f"sag_attn_mass B{B} h{heads} N{N} d{D}", names=("b", "k"))
    assert (got.double().mean(dim=1) - 1.0).abs().max() < tol            # the masses of a sample average 1
    # the mask outside a band equal to the tolerance; at most 10 % of the tokens left out
    near = (ref - 1.0).abs() <= bound
    assert float(near.double().mean()) <= 0.10
    assert bool(((got > 1.0) == (ref > 1.0))[~near].all())
    # bit-reproducible run to run
    again = _launch_mass(sdlib, qkv, B, heads, N, D, extra, exp2)
    assert torch.equal(bits32(got), bits32(again))


def test_attn_mass_refuses_what_its_check_refuses_and_writes_nothing(sdlib):
    B, heads, N, D = 2, 8, 20, 160
    Cc = heads * D
    src = BD.guarded_input(_mass_inputs(B, heads, N, D, 0), torch.bfloat16)
    out = BD.guarded((B, N), torch.float32, fill=3.0)
    base = dict(Q=src.data_ptr(), K=src.data_ptr() + 2 * Cc, ld=3 * Cc, B=B, heads=heads, N=N, D=D)
    for kw in (dict(N=15), dict(N=257), dict(D=40), dict(D=128), dict(heads=0), dict(B=0), dict(ld=2 * Cc - 8), dict(ld=3 * Cc + 4),
               dict(Q=None), dict(K=src.data_ptr() + 2)):
        a = dict(base)
        a.update(kw)
        assert sdlib.sd_op_sag_attn_mass(stream(), a["Q"], a["K"], a["ld"], out.data_ptr(), a["B"], a["heads"], a["N"], a["D"], 0) == -1, kw
        assert sdlib.sd_last_error().decode().startswith("sag_attn_mass:"), (kw, sdlib.sd_last_error())
    torch.cuda.synchronize()
    assert bool((out == 3.0).all())
    BD.check_guards()


# ---------------------------------------------------------------------------------------------------- 2. the degrade op
DEGRADE_SHAPES = [(2, 4, 32, 32), (1, 4, 32, 40), (1, 4, 96, 96), (2, 4, 128, 128)]
A_T = 0.2318            # alphas_cumprod of a mid-schedule step


def _masses(kind, B, mh, mw, g):
    if kind == "mixed":                     # spread round 1, some tokens exactly at the threshold (strict: not blurred)
        m = 0.5 + torch.rand(B, mh * mw, generator=g)
        m[:, ::3] = 1.0
        m[:, 1] = 1.0 + 2.0 ** -23
        return m
    return torch.full((B, mh * mw), 1.25 if kind == "above" else 0.75)


@pytest.mark.parametrize("kind", ["mixed", "above", "below"])
@pytest.mark.parametrize("pred", ["epsilon", "v_prediction", "sample"])
@pytest.mark.parametrize("shape", DEGRADE_SHAPES, ids=[f"{s[0]}x{s[2]}x{s[3]}" for s in DEGRADE_SHAPES])
def test_degrade_per_element(sdlib, shape, pred, kind):
    from sonicdiffusionbayeslab_amd.schedulers import sag_degrade_coef
    B, _, H, W = shape
    mh, mw = H // 8, W // 8
    g = torch.Generator().manual_seed(H * 7 + W + B + so.PRED_IDS[pred])
    x, m = torch.randn(shape, generator=g), torch.randn(shape, generator=g)
    mass = _masses(kind, B, mh, mw, g)
    d = {n: BD.guarded_input(v, label=n) for n, v in (("x", x), ("m", m), ("mass", mass))}
    out = BD.guarded(shape, torch.float32, label="x_deg")
    coef = sag_degrade_coef(pred, A_T)
    _lib.check(sdlib.sd_op_sag_degrade(stream(), d["x"].data_ptr(), d["m"].data_ptr(), d["mass"].data_ptr(), mh, mw, so.PRED_IDS[pred],
                                       (C.c_float * 6)(*coef), out.data_ptr(), B, H, W), "sd_op_sag_degrade")
    torch.cuda.synchronize()
    got = out.cpu().clone()
    BD.check_guards()
    grid = so.mask_of(mass).view(B, mh, mw)
    assert {"mixed": 0 < int(grid.sum()) < grid.numel(), "above": bool(grid.all()), "below": not bool(grid.any())}[kind]
    x64, m64 = x.double(), m.double()
    ref = so.degrade(x64, m64, A_T, pred, grid)
    # the magnitudes along the same path
    sa, s1 = math.sqrt(A_T), math.sqrt(1.0 - A_T)
    c = [abs(v) for v in coef]
    mx0 = c[0] * x64.abs() + c[1] * m64.abs()
    mk = so.upsample8(grid).double()
    mdeg = so.blur(mx0) * mk + mx0 * (1 - mk)
    mag = sa * mdeg + s1 * (c[2] * x64.abs() + c[3] * m64.abs())
    BD.assert_elementwise(got, ref, BD.linear_bound(ref, mag, K_DEGRADE, out=torch.float32), f"sag_degrade {shape} {pred} {kind}",
                          names=("b", "c", "y", "x"))
    if kind == "below":                     # nothing blurred: the noised x0 is the input again (add_noise undoes the split)
        assert rel_l2(got, x) < 1e-5
    if kind == "above":
        assert rel_l2(got, x) > 0.05


def test_degrade_argument_checks(sdlib):
    x = torch.zeros(1, 4, 32, 32, device="cuda")
    mass = torch.ones(1, 16, device="cuda")
    out = torch.full_like(x, 3.0)
    coef = (C.c_float * 6)(1.0, -1.0, 0.0, 1.0, 0.5, 0.5)
    bad = (C.c_float * 6)(1.0, float("nan"), 0.0, 1.0, 0.5, 0.5)

    def run(H=32, W=32, mh=4, mw=4, pred=0, c=coef, o=out.data_ptr(), xs=x.data_ptr()):
        return sdlib.sd_op_sag_degrade(stream(), xs, x.data_ptr(), mass.data_ptr(), mh, mw, pred, c, o, 1, H, W)
    for kw in (dict(H=24), dict(W=136), dict(H=36), dict(mh=5), dict(mw=2), dict(pred=3), dict(pred=-1), dict(c=bad), dict(c=None),
               dict(o=x.data_ptr()), dict(xs=None)):
        assert run(**kw) == -1, kw
        assert sdlib.sd_last_error().decode().startswith("sag_degrade:"), (kw, sdlib.sd_last_error())
    torch.cuda.synchronize()
    assert bool((out == 3.0).all())
    assert run() == 0
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------- 3. the step kernels
STEP_SHAPES = [(2, 4, 8, 8), (3, 4, 8, 8), (2, 4, 20, 4), (3, 4, 20, 4)]       # batch 2 and 3, n_per_sample 256 and 320
STEP_IDS = ["b2-n256", "b3-n256", "b2-n320", "b3-n320"]


def _operands(shape, mode, seed, ncoef):
    g = torch.Generator().manual_seed(seed)
    B = shape[0]
    t = {n: torch.randn(shape, generator=g) for n in ("x", "m1", "m2", "m3", "noise", "x_last", "init", "bnoise")}
    thirds = 3 if mode == GUIDE_CFG_SAG else 2
    t["eps"] = torch.randn((thirds * B,) + tuple(shape[1:]), generator=g)
    t["eps"][-B:] = 0.6 * t["eps"][-B:] + 0.8 * t["eps"][:B]         # d: correlated with the first third, as a UNet's is
    t["k"] = 0.6 + 0.5 * torch.rand(B, generator=g)
    t["mask"] = (torch.rand(B, 1, shape[2], shape[3], generator=g) > 0.5).float()
    t["mask"][:, :, 0, 0], t["mask"][:, :, -1, -1] = 1.0, 0.0
    coef = [f32(v) for v in (torch.rand(ncoef, generator=g) * 2 - 1).tolist()]
    return t, coef


def _guided64(t, mode, gs, s, k=None):
    e = t["eps"].double()
    B = t["x"].shape[0]
    if mode == GUIDE_CFG_SAG:
        u, c, d = e[:B], e[B:2 * B], e[2 * B:]
        v = (u + gs * (c - u)) + s * (u - d)
        m = u.abs() + abs(gs) * (c.abs() + u.abs()) + abs(s) * (u.abs() + d.abs())
    else:
        c, d = e[:B], e[B:]
        v = c + s * (c - d)
        m = c.abs() + abs(s) * (c.abs() + d.abs())
    if k is not None:
        kk = k.double().view(-1, 1, 1, 1)
        v, m = kk * v, kk.abs() * m
    return v, m


def _blend64(t, p, mp, blend):
    a, s = f32(blend[0]), f32(blend[1])
    keep, mkeep = a * t["init"].double() + s * t["bnoise"].double(), abs(a) * t["init"].double().abs() + abs(s) * t["bnoise"].double().abs()
    rep = (t["mask"] >= 0.5).expand_as(p)
    return torch.where(rep, p, keep), torch.where(rep, mp, mkeep)


def _launch_step(sdlib, t, coef, mode, gs, s, use_k, blend):
    d = {n: BD.guarded_input(v, label=n) for n, v in t.items()}
    shape = tuple(t["x"].shape)
    prev, y2, mo = (BD.guarded(shape, torch.float32, label=l) for l in ("prev", "y2", "m_out"))
    n, nps = t["x"].numel(), t["x"][0].numel()
    a, sb = blend if blend is not None else (1.0, 0.0)
    ptr = lambda name: d[name].data_ptr() if blend is not None else None          # noqa: E731
    _lib.check(sdlib.sd_sched_step_sag(stream(), d["eps"].data_ptr(), mode, gs, s, d["x"].data_ptr(), d["m1"].data_ptr(),
                                       d["m2"].data_ptr(), d["m3"].data_ptr(), d["noise"].data_ptr(), prev.data_ptr(), y2.data_ptr(),
                                       mo.data_ptr(), (C.c_float * 10)(*coef), n, d["k"].data_ptr() if use_k else None, nps,
                                       ptr("init"), ptr("bnoise"), ptr("mask"), a, sb, shape[2] * shape[3] if blend is not None else 0),
               "sd_sched_step_sag")
    torch.cuda.synchronize()
    out = [v.cpu().clone() for v in (prev, y2, mo)]
    BD.check_guards()
    return out


@pytest.mark.parametrize("blend", [None, (0.8125 + 2.0 ** -12, 0.58203125 + 2.0 ** -13)], ids=["noblend", "blend"])
@pytest.mark.parametrize("use_k", [False, True], ids=["nok", "k"])
@pytest.mark.parametrize("mode", [GUIDE_CFG_SAG, GUIDE_SAG], ids=["cfg+sag", "sag"])
@pytest.mark.parametrize("shape", STEP_SHAPES, ids=STEP_IDS)
def test_sched_step_sag_per_element(sdlib, shape, mode, use_k, blend):
    t, coef = _operands(shape, mode, seed=sum(shape) * 7 + mode + 2 * use_k, ncoef=10)
    got = _launch_step(sdlib, t, coef, mode, GS, SAG, use_k, blend)
    e, me = _guided64(t, mode, GS, SAG, t["k"] if use_k else None)
    x, m1, m2, m3, z = (t[n].double() for n in ("x", "m1", "m2", "m3", "noise"))
    px, pe, p1, p2, pn, yx, ye, mx, mee, p3 = coef
    prev = px * x + pe * e + p1 * m1 + p2 * m2 + p3 * m3 + pn * z
    mprev = abs(px) * x.abs() + abs(pe) * me + abs(p1) * m1.abs() + abs(p2) * m2.abs() + abs(p3) * m3.abs() + abs(pn) * z.abs()
    if blend is not None:
        prev, mprev = _blend64(t, prev, mprev, blend)
    refs = {"prev": (prev, mprev), "y2": (yx * x + ye * e, abs(yx) * x.abs() + abs(ye) * me),
            "m_out": (mx * x + mee * e, abs(mx) * x.abs() + abs(mee) * me)}
    for name, g in zip(("prev", "y2", "m_out"), got):
        r, m = refs[name]
        BD.assert_elementwise(g, r, BD.linear_bound(r, m, K_STEP, out=torch.float32), f"sched_step_sag {name} {shape} mode {mode} k={use_k}")
    zero = _launch_step(sdlib, t, coef, mode, GS, 0.0, use_k, blend)       # the SAG term is in: the same launch at scale 0 differs
    assert not torch.equal(zero[1], got[1])


@pytest.mark.parametrize("shape", STEP_SHAPES, ids=STEP_IDS)
def test_sag_scale_zero_in_cfg_mode_gives_the_bits_of_sd_sched_step(sdlib, shape):
    t, coef = _operands(shape, GUIDE_CFG_SAG, seed=sum(shape), ncoef=10)
    got = _launch_step(sdlib, t, coef, GUIDE_CFG_SAG, GS, 0.0, False, None)
    B = shape[0]
    d = {n: BD.guarded_input(v, label=n) for n, v in t.items()}
    eps2 = BD.guarded_input(t["eps"][:2 * B], label="eps")
    prev, y2, mo = (BD.guarded(shape, torch.float32, label=l) for l in ("prev", "y2", "m_out"))
    _lib.check(sdlib.sd_sched_step(stream(), eps2.data_ptr(), 1, GS, d["x"].data_ptr(), d["m1"].data_ptr(), d["m2"].data_ptr(),
                                   d["m3"].data_ptr(), d["noise"].data_ptr(), prev.data_ptr(), y2.data_ptr(), mo.data_ptr(),
                                   (C.c_float * 10)(*coef), t["x"].numel()), "sd_sched_step")
    torch.cuda.synchronize()
    for g, w in zip(got, (prev, y2, mo)):
        assert torch.equal(bits32(g), bits32(w.cpu()))
    BD.check_guards()


@pytest.mark.parametrize("variant", ["plain", "k", "k-blend"])
@pytest.mark.parametrize("mode", [GUIDE_CFG_SAG, GUIDE_SAG], ids=["cfg+sag", "sag"])
@pytest.mark.parametrize("shape", STEP_SHAPES, ids=STEP_IDS)
def test_sched_step_pc_sag_per_element(sdlib, shape, mode, variant):
    use_k, blend = "k" in variant, (0.8125 + 2.0 ** -12, 0.58203125 + 2.0 ** -13) if "blend" in variant else None
    t, c = _operands(shape, mode, seed=sum(shape) * 3 + mode + len(variant), ncoef=13)
    d = {n: BD.guarded_input(v, label=n) for n, v in t.items()}
    outs = {n: BD.guarded(shape, torch.float32, label=n) for n in ("prev", "x_corr", "y2", "m_out")}
    a, s = blend if blend is not None else (1.0, 0.0)
    ptr = lambda name: d[name].data_ptr() if blend is not None else None          # noqa: E731
    _lib.check(sdlib.sd_sched_step_pc_sag(stream(), d["eps"].data_ptr(), mode, GS, SAG, d["x"].data_ptr(), d["x_last"].data_ptr(),
                                          d["m1"].data_ptr(), d["m2"].data_ptr(), d["m3"].data_ptr(), outs["prev"].data_ptr(),
                                          outs["x_corr"].data_ptr(), outs["y2"].data_ptr(), outs["m_out"].data_ptr(), (C.c_float * 13)(*c),
                                          t["x"].numel(), d["k"].data_ptr() if use_k else None, t["x"][0].numel(), ptr("init"),
                                          ptr("bnoise"), ptr("mask"), a, s, shape[2] * shape[3] if blend is not None else 0),
               "sd_sched_step_pc_sag")
    torch.cuda.synchronize()
    got = {n: v.cpu().clone() for n, v in outs.items()}
    BD.check_guards()
    e, me = _guided64(t, mode, GS, SAG, t["k"] if use_k else None)
    x, xl, h1, h2, h3 = (t[n].double() for n in ("x", "x_last", "m1", "m2", "m3"))
    cm, cy, cc, cp = c[0:2], c[2:4], c[4:9], c[9:13]
    mt, mmt = cm[0] * x + cm[1] * e, abs(cm[0]) * x.abs() + abs(cm[1]) * me
    y2, my2 = cy[0] * x + cy[1] * e, abs(cy[0]) * x.abs() + abs(cy[1]) * me
    xc = cc[0] * xl + cc[1] * h1 + cc[2] * h2 + cc[3] * h3 + cc[4] * mt
    mxc = abs(cc[0]) * xl.abs() + abs(cc[1]) * h1.abs() + abs(cc[2]) * h2.abs() + abs(cc[3]) * h3.abs() + abs(cc[4]) * mmt
    p = cp[0] * xc + cp[1] * mt + cp[2] * h1 + cp[3] * h2
    mp = abs(cp[0]) * mxc + abs(cp[1]) * mmt + abs(cp[2]) * h1.abs() + abs(cp[3]) * h2.abs()
    if blend is not None:
        p, mp = _blend64(t, p, mp, blend)
    for name, (r, m) in {"prev": (p, mp), "x_corr": (xc, mxc), "y2": (y2, my2), "m_out": (mt, mmt)}.items():
        BD.assert_elementwise(got[name], r, BD.linear_bound(r, m, K_PC, out=torch.float32), f"sched_step_pc_sag {name} {shape} mode {mode} {variant}")


def test_step_argument_checks(sdlib):
    x = torch.zeros(2, 4, 8, 8, device="cuda")
    eps = torch.zeros(6, 4, 8, 8, device="cuda")
    coef = (C.c_float * 10)(*([0.5] * 10))
    coef13 = (C.c_float * 13)(*([0.5] * 5 + [0.0] * 3 + [0.5] * 3 + [0.0] * 2))
    out = torch.full_like(x, 3.0)

    def step(mode=GUIDE_CFG_SAG, gs=GS, s=SAG, n=x.numel(), e=eps.data_ptr(), c=coef):
        return sdlib.sd_sched_step_sag(stream(), e, mode, gs, s, x.data_ptr(), None, None, None, None, out.data_ptr(), None, None, c, n,
                                       None, 0, None, None, None, 1.0, 0.0, 0)

    def step_pc(mode=GUIDE_CFG_SAG, gs=GS, s=SAG, nps=256):
        return sdlib.sd_sched_step_pc_sag(stream(), eps.data_ptr(), mode, gs, s, x.data_ptr(), None, None, None, None, out.data_ptr(),
                                          None, None, None, coef13, x.numel(), None, nps, None, None, None, 1.0, 0.0, 0)
    for call, who in ((step, "sched_step_sag"), (step_pc, "sched_step_pc_sag")):
        for kw, what in ((dict(mode=0), "mode"), (dict(mode=1), "mode"), (dict(mode=2), "mode"), (dict(mode=6), "mode"),
                         (dict(s=float("nan")), "sag_scale"), (dict(s=float("inf")), "sag_scale"), (dict(gs=float("inf")), "guidance")):
            assert call(**kw) == -1, (who, kw)
            msg = sdlib.sd_last_error().decode()
            assert msg.startswith(who + ":") and what in msg, msg
    assert step(n=6) == -1 and "n=6" in sdlib.sd_last_error().decode()
    assert step(e=None) == -1 and "null" in sdlib.sd_last_error().decode()
    assert step(c=None) == -1 and "coefficients" in sdlib.sd_last_error().decode()
    assert step_pc(nps=6) == -1 and "n_per_sample" in sdlib.sd_last_error().decode()
    torch.cuda.synchronize()
    assert bool((out == 3.0).all())
    assert step() == 0 and step_pc() == 0
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------- 4. the UNet
_NETS = {}


def net_of(name):
    from sonicdiffusionbayeslab_amd.unet import HipUNet2DConditionModel
    if name not in _NETS:
        cfg, sd, ocfg, heads = so.env(name)
        _NETS[name] = HipUNet2DConditionModel(cfg, sd)
    return _NETS[name]


def gpu_forward(net, lat, ctx, ub, t, h, w, capture, tile=0, depth=0):
    """(eps, mass [ub, N] or None) of the library; leaves the handle with capture and HyperTile off."""
    net.set_deepcache(-1)
    net.set_hypertile(tile, depth)
    f = 2 ** (len(net.config.block_out_channels) - 1)
    mass = torch.full((ub, (h // f) * (w // f)), float("nan"), device="cuda") if capture else None
    try:
        if capture:
            net.set_sag(True, mass)
        net.set_context(ctx.cuda(), h, w)
        eps = net.forward_latents(lat.cuda(), ub, t).clone()
        torch.cuda.synchronize()
        return eps.cpu(), (mass.cpu() if capture else None)
    finally:
        net.clear_sag()
        net.set_hypertile(0)


@pytest.mark.parametrize("case", so.UNET_CASES, ids=[f"{c[0]}-{c[1]}x{c[2]}" for c in so.UNET_CASES])
def test_capture_leaves_the_forward_alone_and_the_mass_matches_the_oracle(case):
    name, h, w, lb, seed, t = case
    cfg = so.env(name)[0]
    net = net_of(name)
    lat, pe, ne = so.unet_inputs(cfg, h, w, lb, seed)
    ctx = torch.cat([ne, pe])
    ref = so.reference(case)
    off, _ = gpu_forward(net, lat, ctx, 2 * lb, t, h, w, False)
    on, mass = gpu_forward(net, lat, ctx, 2 * lb, t, h, w, True)
    assert torch.equal(bits32(on), bits32(off))                       # capture on = capture off, bit for bit
    assert rel_l2(on, ref["eps"]) < UNET_TOL
    err = float((mass.double() - ref["mass"].double()).abs().max())
    print(f"[sag unet] {name} {h}x{w}: mass against the oracle's, largest difference {err:.4f} (band {ref['band']:.4f} = "
          f"{so.BAND_FACTOR} x the oracle's own shift {ref['shift']:.4f}); mean {float(mass.mean()):.6f}")
    assert torch.isfinite(mass).all() and err <= ref["band"]
    assert (mass.double().mean(dim=1) - 1.0).abs().max() < 1e-3
    so.masks_agree(ref["mass"][:lb], mass[:lb] > 1.0, ref["band"], so.MASK_CAP, f"{name} {h}x{w}")


def test_the_profile_sees_one_more_launch_and_no_other_kind_changes():
    """``forward_profiled`` runs at the UNet's own sample size, so this is the two-level case (32x32, its size): capture adds one
    launch of kind ``sag_mass`` and every other kind keeps its launch count."""
    name, h, w, lb, seed, t = so.UNET_CASES[3]
    cfg = so.env(name)[0]
    assert (h, w) == (cfg.sample_size, cfg.sample_size)
    net = net_of(name)
    lat, pe, ne = so.unet_inputs(cfg, h, w, lb, seed)
    ctx = torch.cat([ne, pe])
    net.set_deepcache(-1)
    net.set_context(ctx.cuda(), h, w)
    plain = net.forward_profiled(lat.cuda(), 2 * lb, t)
    net.set_sag(True, torch.zeros(2 * lb, (h // 2) * (w // 2), device="cuda"))
    try:
        net.set_context(ctx.cuda(), h, w)
        prof = net.forward_profiled(lat.cuda(), 2 * lb, t)
    finally:
        net.clear_sag()
    assert "sag_mass" not in plain and prof["sag_mass"]["launches"] == 1 and prof["sag_mass"]["flops"] > 0
    assert set(prof) == set(plain) | {"sag_mass"}
    for kind in plain:
        assert prof[kind]["launches"] == plain[kind]["launches"], kind


@pytest.mark.parametrize("cfg_on", [False, True], ids=["nocfg", "cfg"])
def test_one_full_sag_step_matches_the_oracle_with_the_library_mask_forced(sdlib, cfg_on):
    """Forward 1 with capture, the degrade op, forward 2 on its own workspace and context, and the combine of the step kernel
    (read back through y2 = e) against the oracle's step with the LIBRARY's mask forced in.

    What is held to UNET_TOL, the bound of ONE UNet output: the degraded latents, the prediction d on them, and e of the step
    without CFG, e = c + s (c - d).  With CFG at 7.5, e = (1 - g + s) u + g c - s d multiplies the errors of u and c by 5.75
    and 7.5 before they meet: the guided prediction of the PLAIN pipeline misses a single forward's bound in the same way (3.7e-2
    here; that is why the loops of tests/test_pipeline_gpu.py are held to FREE_TOL, not UNET_TOL).  In that mode the test holds
    to UNET_TOL what SAG adds -- x_deg and d -- and holds e to the figure that UNET_TOL per UNet output implies for it,
    ``sag_oracle.cfg_step_bound``: UNET_TOL (5.75 |u| + 7.5 |c| + 0.75 |d|) / |e| of the ORACLE's own step, 0.156 at this case,
    computed without the library and asserted in tests/test_sag_cpu.py to lie below the 0.166 that the step moves.  Measured
    with CFG: e 3.5e-2, x_deg 3.3e-3, d 7.0e-3."""
    from sonicdiffusionbayeslab_amd.schedulers import sag_degrade
    from oracle.schedulers import DDIMOracle
    case = so.STEP_CASES[cfg_on]
    name, h, w, lb, seed, t = case
    cfg = so.env(name)[0]
    net = net_of(name)
    lat, pe, ne = so.unet_inputs(cfg, h, w, lb, seed)
    ctx = torch.cat([ne, pe]) if cfg_on else pe
    ub, gs = ctx.shape[0], GS if cfg_on else 1.0
    a = float(DDIMOracle().alphas_cumprod[int(t)])
    mh, mw = h // 8, w // 8
    net.set_deepcache(-1)
    mass = torch.zeros(ub, mh * mw, device="cuda")
    eps = torch.empty(ub + lb, 4, h, w, device="cuda")
    e_dev, prev = torch.empty(lb, 4, h, w, device="cuda"), torch.empty(lb, 4, h, w, device="cuda")
    try:
        net.set_sag(True, mass)
        net.set_context(ctx.cuda(), h, w)
        net.set_sag_context(ctx[:lb].cuda(), h, w)
        x = lat.cuda()
        net.forward_latents(x, ub, t, out=eps[:ub])
        xd = sag_degrade(x, eps[:lb], mass, mh, mw, "epsilon", a)
        net.set_sag(False)
        net.forward_latents(xd, lb, t, out=eps[ub:], sag_forward=True)
        net.set_sag(True)
        again = net.forward_latents(x, ub, t).clone()                  # the first context survived the second forward
        # prev = x, y2 = e: the step kernel's own combine
        _lib.check(sdlib.sd_sched_step_sag(stream(), eps.data_ptr(), GUIDE_CFG_SAG if cfg_on else GUIDE_SAG, gs, SAG, x.data_ptr(), None,
                                           None, None, None, prev.data_ptr(), e_dev.data_ptr(), None,
                                           (C.c_float * 10)(1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0), x.numel(), None, 0, None,
                                           None, None, 1.0, 0.0, 0), "sd_sched_step_sag")
        torch.cuda.synchronize()
    finally:
        net.clear_sag()
    eps, e = eps.cpu(), e_dev.cpu()
    assert torch.equal(bits32(again.cpu()), bits32(eps[:ub]))
    assert rel_l2(e, so.combine(eps[:ub], eps[ub:], lb, cfg_on, gs, SAG)) < 1e-6
    lib_mask = (mass[:lb].cpu() > 1.0).view(lb, mh, mw)
    own = so.step_reference(case, cfg=cfg_on)
    ref = so.step_reference(case, forced_mask=lib_mask, cfg=cfg_on)
    so.masks_agree(own["mass"], lib_mask, own["band"], so.MASK_CAP, f"the SAG step cfg={cfg_on}")
    plain = so.plain_guided(eps[:ub], lb, cfg_on, gs)
    err, moved, err_plain = rel_l2(e, ref["e"]), rel_l2(e, plain), rel_l2(plain, ref["plain"])
    err_x, err_d = rel_l2(xd, ref["x_deg"]), rel_l2(eps[ub:], ref["d"])
    print(f"[sag step] cfg={cfg_on}: e against the oracle's (library mask forced) {err:.3e}; x_deg {err_x:.3e}; d {err_d:.3e}; the plain "
          f"guided prediction against the oracle's {err_plain:.3e}; e against the plain guided prediction {moved:.3f} (floor {so.MOVED_FLOOR})")
    assert err_x < UNET_TOL and err_d < UNET_TOL and rel_l2(eps[:ub], ref["eps1"]) < UNET_TOL
    assert moved >= so.MOVED_FLOOR
    if cfg_on:
        bound = so.cfg_step_bound(own, lb)          # (from the oracle's own step alone: fixed before the library ran)
        print(f"[sag step] cfg: the bound on e that UNET_TOL per UNet output implies {bound:.3e}")
        assert err < bound
    else:
        assert err < UNET_TOL


def test_off_is_off_and_what_the_wrapper_refuses():
    from sonicdiffusionbayeslab_amd.unet import HipUNet2DConditionModel
    cfg, sd, _, _ = so.env("sd15")
    lat, pe, ne = so.unet_inputs(cfg, 32, 32, 1)
    ctx = torch.cat([ne, pe])
    fresh = HipUNet2DConditionModel(cfg, sd)                # a handle that never sees the setting
    fresh.set_deepcache(-1)
    fresh.set_context(ctx.cuda(), 32, 32)
    never = fresh.forward_latents(lat.cuda(), 2, 501.0).clone().cpu()
    never_bytes, never_plans = fresh._workspace_bytes(2, -1, 32, 32), fresh.plan_count()
    net = HipUNet2DConditionModel(cfg, sd)
    before, _ = gpu_forward(net, lat, ctx, 2, 501.0, 32, 32, False)
    plans = net.plan_count()
    gpu_forward(net, lat, ctx, 2, 501.0, 32, 32, True)
    assert net.plan_count() > plans                                   # capture is part of the plan key
    plans = net.plan_count()
    after, _ = gpu_forward(net, lat, ctx, 2, 501.0, 32, 32, False)
    assert torch.equal(before, after) and torch.equal(never, after) and net.plan_count() == plans
    assert net._workspace_bytes(2, -1, 32, 32) == never_bytes and fresh.plan_count() == never_plans
    small = torch.zeros(1, 16, device="cuda")
    net.set_sag(True, small)                                          # a buffer for one sample, a forward of two
    try:
        net.set_context(ctx.cuda(), 32, 32)
        with pytest.raises(_lib.SdHipError, match="mass buffer"):
            net.forward_latents(lat.cuda(), 2, 501.0)
        with pytest.raises(NotImplementedError, match="Token Merging"):
            net.set_tome(0.5)
        with pytest.raises(NotImplementedError, match="SAG"):
            net.set_pag(1)
        net.set_hypertile(8, 3)                                       # tiles the 16x16 mid grid of a 128x128 latent, 2x2
        with pytest.raises(_lib.SdHipError, match="tiles the mid block"):
            net.set_context(ctx.cuda(), 128, 128)
    finally:
        net.set_hypertile(0)
        net.clear_sag()
    torch.cuda.synchronize()
    assert bool((small == 0).all())
    net.set_deepcache(0)
    try:
        with pytest.raises(NotImplementedError, match="DeepCache"):
            net.set_sag(True, small)
    finally:
        net.set_deepcache(-1)


# ------------------------------------------------------------------------------------------------------- 5. the pipeline
PX = 256                            # 256x256 px: 32x32 latents, a 4x4 mid grid


@pytest.fixture(scope="module")
def env():
    from sonicdiffusionbayeslab_amd.models import StableDiffusionModel
    from sonicdiffusionbayeslab_amd.weights import UNetConfig, make_synthetic_state_dict
    cfg = UNetConfig(sample_size=16)
    sd = make_synthetic_state_dict(cfg, seed=1234)
    model = StableDiffusionModel(unet_config=cfg, state_dict=dict(sd)).to("cuda:0")
    return cfg, sd, model


def _sched(model, name, **kw):
    from sonicdiffusionbayeslab_amd.registry import schedulers_registry
    from sonicdiffusionbayeslab_amd.schedulers import PNDMConfigStub
    model.scheduler = schedulers_registry[name].from_config(PNDMConfigStub().config, **kw)
    return model.scheduler


def _inputs(cfg, seed):
    g = torch.Generator().manual_seed(seed)
    lat = torch.randn(1, 4, PX // 8, PX // 8, generator=g)
    pe, ne = (torch.randn(1, cfg.context_len, cfg.cross_attention_dim, generator=g) for _ in range(2))
    return lat, pe, ne


def _sag_call(model, **call):
    """(images of the SAG call, the library's per-step masks, x0 list)."""
    model.enable_sag(SAG)
    model._sag_keep = True
    try:
        out, _, x0s = model(**call)
        masks = [m.cpu() > 1.0 for m in model.sag_masses]
    finally:
        model._sag_keep = False
        model.disable_sag()
    return out.images, masks, x0s


def _gate(name, out, loop_out, plain, lib_masks):
    """``loop_out``: what the oracle loop with the library's masks forced returned."""
    ref, own_masses, bands = loop_out
    err, cs, moved = rel_l2(out, ref), cosine(out, ref), rel_l2(out, plain)
    print(f"[sag pipeline] {name}: rel-L2 {err:.3e} cos {cs:.5f}; against the same call without SAG {moved:.3f}")
    assert len(own_masses) == len(lib_masks)
    for i, (own, got, band) in enumerate(zip(own_masses, lib_masks, bands)):
        so.masks_agree(own, got, band, so.MASK_CAP, f"{name} step {i}")
    assert torch.isfinite(out).all() and err < FREE_TOL and cs > FREE_COS
    assert moved > FREE_TOL                                           # the guidance did something the gate can see


def _ddim_step_fn(o):
    return lambda e, t, x: o.step(e, t, x, return_dict=False)[0]


@pytest.mark.parametrize("cfg_on", [True, False], ids=["cfg", "nocfg"])
def test_ddim_call_matches_the_oracle_loop(env, cfg_on):
    from oracle.schedulers import DDIMOracle
    cfg, sd, model = env
    lat, pe, ne = _inputs(cfg, 91)
    gs = GS if cfg_on else 1.0
    call = dict(prompt_embeds=pe, latents=lat, num_inference_steps=3, guidance_scale=gs, output_type="latent", height=PX, width=PX)
    if cfg_on:
        call["negative_prompt_embeds"] = ne
    _sched(model, "ddim_scheduler")
    model.disable_sag()
    plain, _, _ = model(**call)
    plans = model.unet.plan_count()
    model.enable_sag(SAG)
    try:
        zero, _, _ = model(sag_scale=0.0, **call)
        assert torch.equal(zero.images, plain.images) and model.unet.plan_count() == plans     # sag_scale = 0: the plain call's bits
    finally:
        model.disable_sag()
    out, masks, x0s = _sag_call(model, **call)
    off, _, _ = model(**call)
    assert len(x0s) == 3 and len(masks) == 3 and torch.equal(off.images, plain.images)          # disable_sag(): the plain call's bits
    o = DDIMOracle()
    o.set_timesteps(3)
    ocfg = oracle_cfg(cfg)
    ref = so.loop(sd, ocfg, _ddim_step_fn(o), o.alphas_cumprod, "epsilon", o.timesteps, pe, ne if cfg_on else None, lat, gs, SAG,
                  forced_masks=masks)
    _gate(f"DDIM 3 steps {PX} px cfg={cfg_on}", out, ref, plain.images, masks)


def test_unipc_call_matches_the_oracle_loop(env):
    from tests.test_unipc_gpu import UniPCOracle
    cfg, sd, model = env
    lat, pe, ne = _inputs(cfg, 93)
    kw = dict(solver_order=2, solver_type="bh2")
    call = dict(prompt_embeds=pe, negative_prompt_embeds=ne, latents=lat, num_inference_steps=3, guidance_scale=GS, output_type="latent",
                height=PX, width=PX)
    _sched(model, "unipc_scheduler", **kw)
    plain, _, _ = model(**call)
    _sched(model, "unipc_scheduler", **kw)
    out, masks, _ = _sag_call(model, **call)
    o = UniPCOracle(**kw)
    o.set_timesteps(3)
    ref = so.loop(sd, oracle_cfg(cfg), _ddim_step_fn(o), o.alphas_cumprod, "epsilon", o.timesteps, pe, ne, lat, GS, SAG, forced_masks=masks)
    _gate("UniPC 3 steps", out, ref, plain.images, masks)


def test_image_to_image_call_matches_the_oracle_loop(env):
    """strength 0.6 of 5 DDIM steps: 3 run, from the library's own noised encoding."""
    from oracle.schedulers import DDIMOracle
    cfg, sd, model = env
    _, pe, ne = _inputs(cfg, 95)
    img = torch.rand(1, 3, PX, PX, generator=torch.Generator().manual_seed(96))
    call = dict(prompt_embeds=pe, negative_prompt_embeds=ne, image=img, strength=0.6, num_inference_steps=5, guidance_scale=GS,
                output_type="latent")
    _sched(model, "ddim_scheduler")
    plain, _, _ = model(generator=torch.Generator().manual_seed(97), **call)
    out, masks, x0s = _sag_call(model, generator=torch.Generator().manual_seed(97), **call)
    t_start, steps = model.img2img_steps(5, 0.6)
    assert steps == 3 == len(x0s)
    start = model.img2img_start_latents.cpu()
    o = DDIMOracle()
    o.set_timesteps(5)
    ref = so.loop(sd, oracle_cfg(cfg), _ddim_step_fn(o), o.alphas_cumprod, "epsilon", o.timesteps[t_start:], pe, ne, start, GS, SAG,
                  forced_masks=masks)
    _gate("img2img DDIM strength 0.6 of 5", out, ref, plain.images, masks)


def test_v_prediction_call_on_the_sd2_shaped_unet():
    """Without CFG: on this UNet the oracle's own SAG-against-plain distance is 0.073 then and 0.024 under CFG 7.5, where the
    guidance term dwarfs s (u - d) and the FREE_TOL gate could not see SAG at all (tests/test_sag_cpu.py asserts the 0.073)."""
    from sonicdiffusionbayeslab_amd.models import StableDiffusionModel
    from sonicdiffusionbayeslab_amd.registry import schedulers_registry
    from sonicdiffusionbayeslab_amd.schedulers import PNDMConfigStub
    from tests import sched_ref as R
    cfg, sd, ocfg, heads = so.env("sd2")
    model = StableDiffusionModel(unet_config=cfg, state_dict=dict(sd)).to("cuda:0")
    model.scheduler = schedulers_registry["ddim_scheduler"].from_config(PNDMConfigStub().config, prediction_type="v_prediction")
    lat, pe, ne = _inputs(cfg, 97)
    call = dict(prompt_embeds=pe, latents=lat, num_inference_steps=3, guidance_scale=1.0, output_type="latent", height=PX, width=PX)
    plain, _, _ = model(**call)
    out, masks, _ = _sag_call(model, **call)
    s = model.scheduler
    rs = R.DDIM(torch.from_numpy(s.alphas_cumprod), s._timesteps_list, "v_prediction", s.final_alpha_cumprod)
    ref = so.loop(sd, ocfg, lambda e, t, x: rs.step(e, t, x.double())[0], s.alphas_cumprod, "v_prediction", s._timesteps_list, pe, None,
                  lat, 1.0, SAG, heads_per_level=heads, forced_masks=masks)
    _gate("SD 2.x-shaped, v-prediction, DDIM 3 steps", out, ref, plain.images, masks)


def test_hypertile_below_the_mid_block_composes(env):
    """HyperTile at max_depth 0 tiles level 0 alone: one SAG call against the tiled oracle loop."""
    from oracle.schedulers import DDIMOracle
    import tests.hypertile_oracle as ho
    cfg, sd, model = env
    lat, pe, ne = _inputs(cfg, 99)
    call = dict(prompt_embeds=pe, negative_prompt_embeds=ne, latents=lat, num_inference_steps=3, guidance_scale=GS, output_type="latent",
                height=PX, width=PX)
    _sched(model, "ddim_scheduler")
    model.enable_hypertile(tile_size=64, max_depth=0)
    try:
        plain, _, _ = model(**call)
        out, masks, _ = _sag_call(model, **call)
        tokens = model._hypertile[0]
    finally:
        model.disable_hypertile()
    o = DDIMOracle()
    o.set_timesteps(3)
    ref = so.loop(sd, oracle_cfg(cfg), _ddim_step_fn(o), o.alphas_cumprod, "epsilon", o.timesteps, pe, ne, lat, GS, SAG,
                  forced_masks=masks, tile_fn=lambda: ho.TileRun((PX // 8, PX // 8), tokens))
    _gate("HyperTile max_depth 0 + SAG", out, ref, plain.images, masks)


@pytest.mark.parametrize("name", ["dpm_solver_scheduler", "lcm_scheduler", "pndm_scheduler"])
def test_the_other_schedulers_take_the_sag_step(env, name):
    """DPM-Solver, LCM and PNDM reach the same launcher as DDIM (whose call is held to the oracle loop above): a 3-step call is
    finite, differs from the plain call by more than FREE_TOL, and at ``sag_scale = 0`` is the plain call bit for bit."""
    cfg, sd, model = env
    lat, pe, ne = _inputs(cfg, 101)
    call = dict(prompt_embeds=pe, negative_prompt_embeds=ne, latents=lat, num_inference_steps=3, guidance_scale=GS, output_type="latent",
                height=PX, width=PX)
    seeded = lambda: dict(call, generator=torch.Generator().manual_seed(7))      # noqa: E731  (LCM draws step noise)
    _sched(model, name)
    plain, _, _ = model(**seeded())
    _sched(model, name)
    out, masks, _ = _sag_call(model, **seeded())
    model.enable_sag(SAG)
    try:
        _sched(model, name)
        zero, _, _ = model(sag_scale=0.0, **seeded())
    finally:
        model.disable_sag()
    moved = rel_l2(out, plain.images)
    print(f"[sag pipeline] {name}: against the same call without SAG {moved:.3f}; {len(masks)} UNet evaluations with SAG")
    assert torch.isfinite(out).all() and moved > FREE_TOL and torch.equal(zero.images, plain.images)
    assert len(masks) == (4 if name == "pndm_scheduler" else 3)          # (PNDM evaluates its second timestep twice)


@pytest.mark.parametrize("setting", ["hypertile", "freeu"])
def test_a_plan_setting_toggled_between_two_sag_calls_of_one_size(env, setting):
    """HyperTile or FreeU switched on, off and on again between SAG calls of one batch and size, with no plain call in between:
    the workspace of the SAG forward follows the plans (it is dropped with the main workspace's key), so every call runs and a
    setting gives the same bits whenever it comes round."""
    cfg, sd, model = env
    lat, pe, ne = _inputs(cfg, 103)
    call = dict(prompt_embeds=pe, negative_prompt_embeds=ne, latents=lat, num_inference_steps=2, guidance_scale=GS, output_type="latent",
                height=PX, width=PX)
    on = (lambda: model.enable_hypertile(tile_size=64, max_depth=0)) if setting == "hypertile" else (lambda: model.enable_freeu(0.9, 0.2, 1.2, 1.4))
    off = model.disable_hypertile if setting == "hypertile" else model.disable_freeu
    _sched(model, "ddim_scheduler")
    plain, _, _ = model(**call)                                      # (a plain call first: the SAG workspace starts empty)
    model.enable_sag(SAG)
    try:
        outs = []
        for state in (True, False, True, False):
            (on if state else off)()
            outs.append(model(**call)[0].images.clone())
            assert model.unet._sag_ws.tensor is not None and model.unet._sag_ctx_key is not None
    finally:
        off()
        model.disable_sag()
    assert all(torch.isfinite(o).all() for o in outs)
    assert torch.equal(outs[0], outs[2]) and torch.equal(outs[1], outs[3]) and not torch.equal(outs[0], outs[1])
    assert rel_l2(outs[1], plain.images) > FREE_TOL
    after, _, _ = model(**call)
    assert torch.equal(after.images, plain.images)
