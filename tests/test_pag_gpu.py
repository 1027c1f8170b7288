"""Perturbed-attention guidance on the GPU: the PAG forms of the step kernels and of the rescale factors per element against fp64
restatements, the identity self-attention kernel of csrc/pag.hip bit for bit against the index map of its definition, the UNet
forward against the PAG oracle (tests/pag_oracle.py), and the pipeline against the oracle loop.

Tolerances.  The step kernels: tests/bounds.py's rule for an fp32 output -- one ulp plus 2^-24 K mag -- with K the longest
input-to-output path as tests/test_unipc_gpu.py counts it, three operations longer for the PAG term (c - p, s * (.), + (.)).  The
identity op is a copy: bit-exact.  The UNet: UNET_TOL of tests/test_unet_gpu.py against the oracle, the unperturbed samples also
against the library's own plain forward, and -- so that this means the perturbation happened -- the perturbed third at least
FLOOR = 5 x UNET_TOL away from the cond third (tests/test_pag_cpu.py holds the oracle's own distance to the same floor at the
same inputs).  The pipeline: FREE_TOL / FREE_COS of tests/test_pipeline_gpu.py."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

from sonicdiffusionbayeslab_amd import _lib
from tests import bounds as BD
from tests import pag_oracle as po
from tests.util import cosine, oracle_cfg, rel_l2, synth_inputs

UNET_TOL = 2e-2                     # tests/test_unet_gpu.py
FREE_TOL, FREE_COS = 6e-2, 0.998    # tests/test_pipeline_gpu.py
GUIDE_CFG_PAG, GUIDE_PAG = 2, 3     # include/sd_hip.h
GS, PAG = 7.5, 3.0
# sd_sched_step_pag, eps -> prev with CFG, PAG and k:  c - u, g * (.), u + (.)  [3];  c - p, s * (.), + (.)  [3];  k[b] * e  [1];
# pe * e, (px x) + (.), + p1 m1, + p2 m2, + p3 m3, + pn noise  [6]  = 13.  sd_sched_step_pc_pag: tests/test_unipc_gpu.py's 12 + 3.
K_STEP, K_PC = 13, 15


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


# ------------------------------------------------------------------------------------------------ 1. the step kernels
STEP_SHAPES = [(2, 4, 8, 8), (3, 4, 8, 8), (2, 4, 20, 4), (3, 4, 20, 4)]       # batch 2 and 3, n_per_sample 256 and 4 * 20 * 4
STEP_IDS = ["b2-n256", "b3-n256", "b2-n320", "b3-n320"]


def _operands(shape, mode, seed, ncoef):
    g = torch.Generator().manual_seed(seed)
    B = shape[0]
    t = {n: torch.randn(shape, generator=g) for n in ("x", "m1", "m2", "m3", "noise", "x_last", "init", "bnoise")}
    thirds = 3 if mode == GUIDE_CFG_PAG else 2
    t["eps"] = torch.randn((thirds * B,) + tuple(shape[1:]), generator=g)
    t["eps"][-2 * B:-B] = 1.7 * t["eps"][-2 * B:-B] + 0.3            # the cond third: another scale and mean
    t["eps"][-B:] = 0.6 * t["eps"][-B:] + 0.8 * t["eps"][-2 * B:-B]  # the perturbed third: correlated with it, as a UNet's is
    t["k"] = 0.6 + 0.5 * torch.rand(B, generator=g)
    t["mask"] = (torch.rand(B, 1, shape[2], shape[3], generator=g) > 0.5).float()
    t["mask"][:, :, 0, 0], t["mask"][:, :, -1, -1] = 1.0, 0.0          # both sides of the blend in every sample
    coef = [f32(v) for v in (torch.rand(ncoef, generator=g) * 2 - 1).tolist()]
    return t, coef


def _guided64(t, mode, gs, pag, k=None):
    """(e, |e| chain) in fp64 from the fp32 thirds, in the documented order."""
    e = t["eps"].double()
    B = t["x"].shape[0]
    if mode == GUIDE_CFG_PAG:
        u, c, p = e[:B], e[B:2 * B], e[2 * B:]
        v = (u + gs * (c - u)) + pag * (c - p)
        m = u.abs() + abs(gs) * (c.abs() + u.abs()) + abs(pag) * (c.abs() + p.abs())
    else:
        c, p = e[:B], e[B:]
        v = c + pag * (c - p)
        m = c.abs() + abs(pag) * (c.abs() + p.abs())
    if k is not None:
        kk = k.double().view(-1, 1, 1, 1)
        v, m = kk * v, kk.abs() * m
    return v, m


def _blend64(t, p, mp, blend):
    a, s = f32(blend[0]), f32(blend[1])
    keep, mkeep = a * t["init"].double() + s * t["bnoise"].double(), abs(a) * t["init"].double().abs() + abs(s) * t["bnoise"].double().abs()
    rep = (t["mask"] >= 0.5).expand_as(p)
    return torch.where(rep, p, keep), torch.where(rep, mp, mkeep)


def _launch_step(sdlib, t, coef, mode, gs, pag, use_k, blend):
    d = {n: BD.guarded_input(v, label=n) for n, v in t.items()}
    shape = tuple(t["x"].shape)
    prev, y2, mo = (BD.guarded(shape, torch.float32, label=l) for l in ("prev", "y2", "m_out"))
    n, nps = t["x"].numel(), t["x"][0].numel()
    a, s = blend if blend is not None else (1.0, 0.0)
    ptr = lambda name: d[name].data_ptr() if blend is not None else None          # noqa: E731
    _lib.check(sdlib.sd_sched_step_pag(stream(), d["eps"].data_ptr(), mode, gs, pag, d["x"].data_ptr(), d["m1"].data_ptr(),
                                       d["m2"].data_ptr(), d["m3"].data_ptr(), d["noise"].data_ptr(), prev.data_ptr(), y2.data_ptr(),
                                       mo.data_ptr(), (C.c_float * 10)(*coef), n, d["k"].data_ptr() if use_k else None, nps,
                                       ptr("init"), ptr("bnoise"), ptr("mask"), a, s, shape[2] * shape[3] if blend is not None else 0),
               "sd_sched_step_pag")
    torch.cuda.synchronize()
    out = [v.cpu().clone() for v in (prev, y2, mo)]
    BD.check_guards()
    return out


@pytest.mark.parametrize("blend", [None, (0.8125 + 2.0 ** -12, 0.58203125 + 2.0 ** -13)], ids=["noblend", "blend"])
@pytest.mark.parametrize("use_k", [False, True], ids=["nok", "k"])
@pytest.mark.parametrize("mode", [GUIDE_CFG_PAG, GUIDE_PAG], ids=["cfg+pag", "pag"])
@pytest.mark.parametrize("shape", STEP_SHAPES, ids=STEP_IDS)
def test_sched_step_pag_per_element(sdlib, shape, mode, use_k, blend):
    t, coef = _operands(shape, mode, seed=sum(shape) * 7 + mode + 2 * use_k, ncoef=10)
    got = _launch_step(sdlib, t, coef, mode, GS, PAG, use_k, blend)
    e, me = _guided64(t, mode, GS, PAG, t["k"] if use_k else None)
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
        BD.assert_elementwise(g, r, BD.linear_bound(r, m, K_STEP, out=torch.float32), f"sched_step_pag {name} {shape} mode {mode} k={use_k}")
    # the PAG term is in: the same launch at scale 0 differs
    zero = _launch_step(sdlib, t, coef, mode, GS, 0.0, use_k, blend)
    assert not torch.equal(zero[1], got[1])


@pytest.mark.parametrize("shape", STEP_SHAPES, ids=STEP_IDS)
def test_pag_scale_zero_in_cfg_mode_gives_the_bits_of_sd_sched_step(sdlib, shape):
    t, coef = _operands(shape, GUIDE_CFG_PAG, seed=sum(shape), ncoef=10)
    got = _launch_step(sdlib, t, coef, GUIDE_CFG_PAG, GS, 0.0, False, None)
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
@pytest.mark.parametrize("mode", [GUIDE_CFG_PAG, GUIDE_PAG], ids=["cfg+pag", "pag"])
@pytest.mark.parametrize("shape", STEP_SHAPES, ids=STEP_IDS)
def test_sched_step_pc_pag_per_element(sdlib, shape, mode, variant):
    use_k, blend = "k" in variant, (0.8125 + 2.0 ** -12, 0.58203125 + 2.0 ** -13) if "blend" in variant else None
    t, c = _operands(shape, mode, seed=sum(shape) * 3 + mode + len(variant), ncoef=13)
    d = {n: BD.guarded_input(v, label=n) for n, v in t.items()}
    outs = {n: BD.guarded(shape, torch.float32, label=n) for n in ("prev", "x_corr", "y2", "m_out")}
    a, s = blend if blend is not None else (1.0, 0.0)
    ptr = lambda name: d[name].data_ptr() if blend is not None else None          # noqa: E731
    _lib.check(sdlib.sd_sched_step_pc_pag(stream(), d["eps"].data_ptr(), mode, GS, PAG, d["x"].data_ptr(), d["x_last"].data_ptr(),
                                          d["m1"].data_ptr(), d["m2"].data_ptr(), d["m3"].data_ptr(), outs["prev"].data_ptr(),
                                          outs["x_corr"].data_ptr(), outs["y2"].data_ptr(), outs["m_out"].data_ptr(), (C.c_float * 13)(*c),
                                          t["x"].numel(), d["k"].data_ptr() if use_k else None, t["x"][0].numel(), ptr("init"),
                                          ptr("bnoise"), ptr("mask"), a, s, shape[2] * shape[3] if blend is not None else 0),
               "sd_sched_step_pc_pag")
    torch.cuda.synchronize()
    got = {n: v.cpu().clone() for n, v in outs.items()}
    BD.check_guards()
    e, me = _guided64(t, mode, GS, PAG, t["k"] if use_k else None)
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
        BD.assert_elementwise(got[name], r, BD.linear_bound(r, m, K_PC, out=torch.float32), f"sched_step_pc_pag {name} {shape} mode {mode} {variant}")


@pytest.mark.parametrize("r", [0.3, 0.7])
@pytest.mark.parametrize("shape", STEP_SHAPES, ids=STEP_IDS)
def test_rescale_factors_pag_per_element_and_in_the_step(sdlib, shape, r):
    """k_b = r std(c_b) / std(e_b) + (1 - r) with e including the PAG term; the bound is tests/test_rescale_gpu.py's, with the
    three further roundings of the PAG term in the error of e."""
    U = 2.0 ** -24
    t, coef = _operands(shape, GUIDE_CFG_PAG, seed=sum(shape) + int(10 * r), ncoef=10)
    B, nps = shape[0], t["x"][0].numel()
    eps = BD.guarded_input(t["eps"], label="eps")
    k = BD.guarded((B,), torch.float32, label="k")
    _lib.check(sdlib.sd_cfg_rescale_factors_pag(stream(), eps.data_ptr(), B, nps, GS, PAG, r, k.data_ptr()), "sd_cfg_rescale_factors_pag")
    torch.cuda.synchronize()
    got = k.cpu().clone()
    BD.check_guards()
    e64 = t["eps"].double()
    u, c, p = e64[:B], e64[B:2 * B], e64[2 * B:]
    gcfg = u + GS * (c - u)
    e = gcfg + PAG * (c - p)
    dims = (1, 2, 3)
    want = (r * c.std(dim=dims) / e.std(dim=dims) + (1.0 - r))
    Ee = U * (2.0 * GS * (c - u).abs() + gcfg.abs() + 2.0 * PAG * (c - p).abs() + e.abs()) * (1 + 1e-6)
    ec = e - e.mean(dim=dims, keepdim=True)
    ds = Ee.pow(2).sum(dim=dims).sqrt() / ec.pow(2).sum(dim=dims).sqrt() + 1e-12
    bound = r * ((want - (1.0 - r)) / r) * (ds / (1 - ds)) * 1.01 + BD.ulp_fp32(want)
    BD.assert_elementwise(got, want, bound, f"cfg_rescale_factors_pag {shape} r={r}")
    # ... it is not the plain factor, and at scale 0 it is, bit for bit
    k0, kp = BD.guarded((B,), torch.float32), BD.guarded((B,), torch.float32)
    eps2 = BD.guarded_input(t["eps"][:2 * B])
    _lib.check(sdlib.sd_cfg_rescale_factors_pag(stream(), eps.data_ptr(), B, nps, GS, 0.0, r, k0.data_ptr()))
    _lib.check(sdlib.sd_cfg_rescale_factors(stream(), eps2.data_ptr(), B, nps, GS, r, kp.data_ptr()))
    torch.cuda.synchronize()
    assert torch.equal(bits32(k0.cpu()), bits32(kp.cpu())) and not torch.equal(got, kp.cpu())
    BD.check_guards()
    # the product's step with guidance_rescale: rescale_noise_cfg(e, c, r) with e including the PAG term
    from sonicdiffusionbayeslab_amd.registry import schedulers_registry
    from sonicdiffusionbayeslab_amd.schedulers import PNDMConfigStub
    sch = schedulers_registry["ddim_scheduler"].from_config(PNDMConfigStub().config)
    sch.set_timesteps(10, device="cuda")
    ts = sch._timesteps_list[3]
    prev, x0 = sch.step_fused(t["eps"].cuda(), GS, t["x"].cuda(), ts, cfg=True, guidance_rescale=r, pag_scale=PAG)
    cx, ce, dx, de = sch.coefficients(ts)
    ek = want.view(-1, 1, 1, 1) * e
    assert rel_l2(prev, cx * t["x"].double() + ce * ek) < 1e-5 and rel_l2(x0, dx * t["x"].double() + de * ek) < 1e-5
    assert rel_l2(po.guided(t["eps"], B, True, GS, PAG, r), ek) < 1e-5          # the oracle's own combine says the same


def test_step_argument_checks(sdlib):
    x = torch.zeros(2, 4, 8, 8, device="cuda")
    eps = torch.zeros(6, 4, 8, 8, device="cuda")
    coef = (C.c_float * 10)(*([0.5] * 10))
    coef13 = (C.c_float * 13)(*([0.5] * 5 + [0.0] * 3 + [0.5] * 3 + [0.0] * 2))       # (null history entries carry no weight)
    out = torch.full_like(x, 3.0)

    def step(mode=GUIDE_CFG_PAG, gs=GS, pag=PAG, n=x.numel(), e=eps.data_ptr(), c=coef):
        return sdlib.sd_sched_step_pag(stream(), e, mode, gs, pag, x.data_ptr(), None, None, None, None, out.data_ptr(), None, None, c, n,
                                       None, 0, None, None, None, 1.0, 0.0, 0)

    def step_pc(mode=GUIDE_CFG_PAG, gs=GS, pag=PAG, nps=256):
        return sdlib.sd_sched_step_pc_pag(stream(), eps.data_ptr(), mode, gs, pag, x.data_ptr(), None, None, None, None, out.data_ptr(),
                                          None, None, None, coef13, x.numel(), None, nps, None, None, None, 1.0, 0.0, 0)
    for call, who in ((step, "sched_step_pag"), (step_pc, "sched_step_pc_pag")):
        for kw, what in ((dict(mode=0), "mode"), (dict(mode=1), "mode"), (dict(mode=4), "mode"), (dict(pag=float("nan")), "pag_scale"),
                         (dict(pag=float("inf")), "pag_scale"), (dict(gs=float("inf")), "guidance")):
            assert call(**kw) == -1, (who, kw)
            msg = sdlib.sd_last_error().decode()
            assert msg.startswith(who + ":") and what in msg, msg
    assert step(n=6) == -1 and "n=6" in sdlib.sd_last_error().decode()
    assert step(e=None) == -1 and "null" in sdlib.sd_last_error().decode()
    assert step(c=None) == -1 and "coefficients" in sdlib.sd_last_error().decode()
    assert step_pc(nps=6) == -1 and "n_per_sample" in sdlib.sd_last_error().decode()
    k = torch.zeros(2, device="cuda")
    assert sdlib.sd_cfg_rescale_factors_pag(stream(), eps.data_ptr(), 2, 256, GS, float("nan"), 0.7, k.data_ptr()) == -1
    assert "pag_scale" in sdlib.sd_last_error().decode()
    assert sdlib.sd_cfg_rescale_factors_pag(stream(), eps.data_ptr(), 2, 6, GS, PAG, 0.7, k.data_ptr()) == -1
    torch.cuda.synchronize()
    assert bool((out == 3.0).all())
    assert step() == 0 and step_pc() == 0
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 2. the identity op
#              N (tokens)  C     heads  head-major
IDENTITY = [(4, 1280, 8, False), (64, 640, 8, False), (256, 320, 8, False), (256, 320, 5, False),
            (256, 320, 8, True), (1024, 320, 8, True)]


def bits16(t):
    return t.contiguous().view(torch.int16).cpu()


@pytest.mark.parametrize("B_total,n_pert", [(3, 1), (6, 2)], ids=["3-last1", "6-last2"])
@pytest.mark.parametrize("N,Cc,heads,hm", IDENTITY, ids=[f"N{c[0]}-C{c[1]}-h{c[2]}-{'hm' if c[3] else 'tm'}" for c in IDENTITY])
def test_identity_op_is_bit_exact_with_guard_bands(sdlib, N, Cc, heads, hm, B_total, n_pert):
    D = Cc // heads
    g = torch.Generator().manual_seed(N + Cc + heads + B_total)
    qkv = torch.randn(B_total, N, 3 * Cc, generator=g).to(torch.bfloat16)
    qkv[B_total - 1, 0, 2 * Cc:2 * Cc + 4] = torch.tensor([0.0, -0.0, float("inf"), float("nan")], dtype=torch.bfloat16)
    v = qkv[:, :, 2 * Cc:]                                          # [B, N, C]
    rows_total, row0, rows = B_total * N, (B_total - n_pert) * N, n_pert * N
    # the index map of the definition: out[r][h * D + d] = V(r, h, d)
    want = torch.full((rows_total, Cc), 3.0, dtype=torch.bfloat16)
    want[row0:] = v.reshape(rows_total, Cc)[row0:]
    out = BD.guarded((rows_total, Cc), torch.bfloat16, fill=3.0)
    if hm:
        vh = v.reshape(B_total, N, heads, D).permute(0, 2, 1, 3).contiguous()       # [sample][head][token][D]
        for (b, h, tk, d) in ((B_total - 1, heads - 1, N - 1, D - 1), (B_total - n_pert, 1, 5, 3)):
            assert vh[b, h, tk, d].item() == want[b * N + tk, h * D + d].item() or vh[b, h, tk, d].isnan()
        src = BD.guarded_input(vh.reshape(B_total * heads * N, D), torch.bfloat16)
        _lib.check(sdlib.sd_op_pag_identity(stream(), src.data_ptr(), 0, N, out.data_ptr(), rows_total, row0, rows, Cc, heads), "sd_op_pag_identity")
    else:
        src = BD.guarded_input(qkv.reshape(rows_total, 3 * Cc), torch.bfloat16)
        _lib.check(sdlib.sd_op_pag_identity(stream(), src.data_ptr() + 2 * Cc * 2, 3 * Cc, 0, out.data_ptr(), rows_total, row0, rows, Cc, heads),
                   "sd_op_pag_identity")
    torch.cuda.synchronize()
    assert torch.equal(bits16(out), bits16(want))                      # the perturbed rows are V's bits, the others untouched
    BD.check_guards()


def test_identity_op_refuses_what_its_check_refuses_and_writes_nothing(sdlib):
    N, Cc, heads = 64, 320, 8
    src = BD.guarded_input(torch.randn(3 * N, 3 * Cc).to(torch.bfloat16), torch.bfloat16)
    out = BD.guarded((3 * N, Cc), torch.bfloat16, fill=3.0)
    base = dict(V=src.data_ptr() + 4 * Cc, ldv=3 * Cc, tok=0, rows_total=3 * N, row0=2 * N, rows=N, C=Cc, heads=heads)
    for kw in (dict(rows=N + 1), dict(row0=-1), dict(rows=0), dict(C=324), dict(heads=3), dict(ldv=312), dict(tok=48), dict(tok=-1),
               dict(V=None), dict(V=src.data_ptr() + 2)):
        a = dict(base)
        a.update(kw)
        assert sdlib.sd_op_pag_identity(stream(), a["V"], a["ldv"], a["tok"], out.data_ptr(), a["rows_total"], a["row0"], a["rows"], a["C"],
                                        a["heads"]) == -1, kw
        assert sdlib.sd_last_error().decode().startswith("pag_identity:"), (kw, sdlib.sd_last_error())
    torch.cuda.synchronize()
    assert bool((out == 3.0).all())
    BD.check_guards()


# ------------------------------------------------------------------------------------------------------------- 3. the UNet
_NETS = {}


def net_of(name):
    import os
    from sonicdiffusionbayeslab_amd.unet import HipUNet2DConditionModel
    if name not in _NETS:
        cfg, sd, ocfg, heads = po.env(name)
        os.environ["SD_DEBUG_TAPS"] = "1"
        try:
            _NETS[name] = HipUNet2DConditionModel(cfg, sd)
        finally:
            os.environ.pop("SD_DEBUG_TAPS")
    return _NETS[name]


def gpu_forward(net, lat, ctx, ub, t, h, w, mask, tile=0, tap=None):
    """eps of the library with the PAG layer mask (0 = off) and HyperTile at ``tile`` tokens; leaves the handle with both off."""
    net.set_deepcache(-1)
    net.set_hypertile(tile, 0)
    net.set_pag(mask)
    try:
        net.set_context(ctx.cuda(), h, w)
        eps = net.forward_latents(lat.cuda(), ub, t).clone()
        torch.cuda.synchronize()
        if tap is not None:
            c = net.config.block_out_channels[-1]
            hh, ww = h >> (len(net.config.block_out_channels) - 1), w >> (len(net.config.block_out_channels) - 1)
            tap_t = net.debug_tensor(tap, ub, ub * hh * ww * c, h, w).view(ub, hh, ww, c).permute(0, 3, 1, 2)
            return eps.cpu(), tap_t
        return eps.cpu()
    finally:
        net.set_pag(0)
        net.set_hypertile(0)


def forward_pag_and_check(case, rep, tile=0):
    from sonicdiffusionbayeslab_amd.unet import HipUNet2DConditionModel as U
    name, h, w, lb, seed, t, layers, n = case
    cfg = po.env(name)[0]
    net = net_of(name)
    ub = rep * lb
    lat, ctx, _ = po.unet_inputs(cfg, h, w, lb, rep, seed)
    ref = po.reference(case, rep, tile)
    mask = U.pag_layer_mask(cfg, list(layers))
    assert bin(mask).count("1") == n == len(ref["used"])
    eps = gpu_forward(net, lat, ctx, ub, t, h, w, mask, tile)
    own_plain = gpu_forward(net, lat, ctx[:-lb], ub - lb, t, h, w, 0, tile)
    err, err_plain = rel_l2(eps, ref["eps"]), rel_l2(eps[:-lb], own_plain)
    err_pert = rel_l2(eps[-lb:], ref["eps"][-lb:])
    moved, own = rel_l2(eps[-lb:], eps[-2 * lb:-lb]), rel_l2(ref["eps"][-lb:], ref["eps"][-2 * lb:-lb])
    print(f"[pag unet] {name} {h}x{w} lb {lb} x{rep} {layers} tile {tile}: rel-L2 vs the PAG oracle {err:.3e} (perturbed third {err_pert:.3e}) "
          f"cos {cosine(eps, ref['eps']):.5f}; unperturbed vs the library's plain forward {err_plain:.3e}; perturbed vs cond {moved:.3f} "
          f"(the oracle's own {own:.3f}, floor {po.FLOOR:.2f})")
    assert own > po.FLOOR
    assert torch.isfinite(eps).all() and err < UNET_TOL and err_pert < UNET_TOL
    assert err_plain < UNET_TOL and rel_l2(own_plain, ref["plain"]) < UNET_TOL
    assert moved > po.FLOOR
    return net, lat, ctx, mask


def _ids(cases):
    return ["+".join(c[6]) for c in cases]


SD15 = [c for c in po.UNET_CASES if c[0] == "sd15"]
TWO_LEVEL = [c for c in po.UNET_CASES if c[0] == "two_level"]


@pytest.mark.parametrize("rep", [3, 2], ids=["ub3lb", "ub2lb"])
@pytest.mark.parametrize("case", SD15, ids=_ids(SD15))
def test_unet_forward_matches_the_pag_oracle(case, rep):
    """16x16 latents, 2 latents, [uncond | cond | perturbed] and [cond | perturbed].  The two cases that name
    down_blocks.0.attentions.0 exercise the prefix rule: the prompt-independent prefix ends at that block's entry."""
    net, lat, ctx, mask = forward_pag_and_check(case, rep)
    name, h, w, lb, seed, t, layers, n = case
    net.set_pag(mask)
    try:
        net.set_context(ctx.cuda(), h, w)
        prof = net.forward_profiled(lat.cuda(), rep * lb, t)
    finally:
        net.set_pag(0)
    assert prof["pag_identity"]["launches"] == n and prof["pag_identity"]["bytes"] > 0
    net.set_context(ctx.cuda(), h, w)
    plain = net.forward_profiled(lat.cuda(), rep * lb, t)
    assert "pag_identity" not in plain
    # to_out stays one GEMM and attn1 one launch per block: the same launch count of every other kind but the replicate's
    for kind in ("gemm", "attention", "layernorm", "xattn_fused", "conv3x3"):
        assert prof.get(kind, {"launches": 0})["launches"] == plain.get(kind, {"launches": 0})["launches"], kind


HEAD_MAJOR = [(TWO_LEVEL[0], 3, False), (TWO_LEVEL[0], 2, False), (po.HM_CASE, 3, True)]


@pytest.mark.parametrize("case,rep,hm", HEAD_MAJOR, ids=["lb2-ub6-token-major", "lb2-ub4-token-major", "lb3-ub9-head-major"])
def test_unet_forward_on_and_off_the_head_major_path(sdlib, case, rep, hm):
    """32x32 latents on the 320 / 640 UNet: the five perturbed blocks sit on level 0, 1024 tokens (the fused prompt
    cross-attention).  The q|k|v projection stores K / V head-major, and the identity op reads V from that layout, when the
    predicate of csrc/plan.hip (Builder::transformer_block) holds -- which needs 128-row GEMM tiles, from 8192 rows on: 3 latents
    x 3 (9216 rows) take it, 2 latents (6144 and 4096 rows) stay token-major at the same token count.  The first block is
    perturbed, so the prefix ends at its entry and every block sees the full batch."""
    name, h, w, lb, seed, t, layers, n = case
    cfg = po.env(name)[0]
    Cc, heads, M = cfg.block_out_channels[0], cfg.num_heads, rep * lb * h * w
    assert Cc // heads == 40 and Cc % 160 == 0 and (h * w) % 128 == 0 and h * w >= 256 and sdlib.sd_op_gemm_splitk(M, 3 * Cc, Cc, 0) == 1
    assert (sdlib.sd_op_gemm_tile_rows(M, 3 * Cc, 0) == 128) == hm
    forward_pag_and_check(case, rep)


def test_sd2_shaped_unet_forward():
    """The SD 2.x-shaped UNet (5 / 10 / 20 / 20 heads of 64) at 16x16."""
    forward_pag_and_check(po.SD2_CASE, 3)


def test_unet_forward_with_hypertile():
    """HyperTile at T = 8 (level 0 in 2x2 tiles) with a tiled perturbed block among the layers: the perturbed rows stay last."""
    forward_pag_and_check(po.HT_CASE, 3, po.HT_TOKENS)


def test_default_layer_set_at_the_mid_tensor():
    """``"mid"`` alone moves the output less than the floor (0.025), so the comparison is made at the "mid" debug tensor."""
    from sonicdiffusionbayeslab_amd.unet import HipUNet2DConditionModel as U
    name, h, w, lb, seed, t, layers, n = po.MID_CASE
    cfg = po.env(name)[0]
    net = net_of(name)
    lat, ctx, _ = po.unet_inputs(cfg, h, w, lb, 3, seed)
    ref = po.reference(po.MID_CASE)
    eps, mid = gpu_forward(net, lat, ctx, 3 * lb, t, h, w, U.pag_layer_mask(cfg, "mid"), tap="mid")
    _, mid_plain = gpu_forward(net, lat, ctx[:-lb], 2 * lb, t, h, w, 0, tap="mid")
    err, moved = rel_l2(mid, ref["mid"]), rel_l2(mid[-lb:], mid[-2 * lb:-lb])
    own = rel_l2(ref["mid"][-lb:], ref["mid"][-2 * lb:-lb])
    print(f"[pag unet] 'mid' at the mid tensor: rel-L2 vs the oracle {err:.3e}; perturbed vs cond {moved:.3f} (the oracle's own {own:.3f}, "
          f"floor {po.MID_FLOOR:.2f}); output vs the oracle {rel_l2(eps, ref['eps']):.3e}")
    assert own > po.MID_FLOOR and moved > po.MID_FLOOR
    assert err < UNET_TOL and rel_l2(mid[-lb:], ref["mid"][-lb:]) < UNET_TOL and rel_l2(eps, ref["eps"]) < UNET_TOL
    assert rel_l2(mid[:-lb], mid_plain) < UNET_TOL


def test_off_is_off_and_the_forward_refuses_other_batches():
    from sonicdiffusionbayeslab_amd.unet import HipUNet2DConditionModel
    cfg, sd, _, _ = po.env("sd15")
    lat, pe, ne = synth_inputs(cfg, 1)
    ctx = torch.cat([ne, pe])
    fresh = HipUNet2DConditionModel(cfg, sd)                # a handle that never sees the setting
    fresh.set_deepcache(-1)
    fresh.set_context(ctx.cuda())
    never = fresh.forward_latents(lat.cuda(), 2, 501.0).clone().cpu()
    never_bytes, never_plans = fresh._workspace_bytes(2, -1, 16, 16), fresh.plan_count()
    net = HipUNet2DConditionModel(cfg, sd)                  # (no debug taps: its workspace is the fresh handle's)
    before = gpu_forward(net, lat, ctx, 2, 501.0, 16, 16, 0)
    plans = net.plan_count()
    gpu_forward(net, lat, torch.cat([ctx, pe]), 3, 501.0, 16, 16, 1 << 6)
    assert net.plan_count() > plans
    plans = net.plan_count()
    after = gpu_forward(net, lat, ctx, 2, 501.0, 16, 16, 0)
    assert torch.equal(before, after) and torch.equal(never, after) and net.plan_count() == plans
    assert net._workspace_bytes(2, -1, 16, 16) == never_bytes and fresh.plan_count() == never_plans
    # with a mask set the forward takes 3 or 2 copies of the latents, nothing else, and no DeepCache
    net.set_pag(1 << 6)
    try:
        net.set_context(torch.cat([ctx, ctx]).cuda())
        with pytest.raises(_lib.SdHipError, match="3 or 2 times"):
            net.forward_latents(lat.cuda(), 4, 501.0)
        with pytest.raises(NotImplementedError, match="Token Merging"):
            net.set_tome(0.5)
    finally:
        net.set_pag(0)
    with pytest.raises(ValueError, match="layer_mask"):
        net.set_pag(1 << 16)
    net.set_deepcache(0)
    try:
        with pytest.raises(NotImplementedError, match="DeepCache"):
            net.set_pag(1)
    finally:
        net.set_deepcache(-1)


# ------------------------------------------------------------------------------------------------------- 4. the pipeline
PX = 256                            # 256x256 px: 32x32 latents on the UNet whose own size is 16x16
LAYERS = ["mid", "up.block_1"]


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


def _gate(name, out, ref, plain):
    err, cs, moved = rel_l2(out, ref), cosine(out, ref), rel_l2(out, plain)
    print(f"[pag pipeline] {name}: rel-L2 {err:.3e} cos {cs:.5f}; against the same call without PAG {moved:.3f}")
    assert torch.isfinite(out).all() and err < FREE_TOL and cs > FREE_COS
    assert moved > FREE_TOL                                           # the guidance did something the gate can see


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
    model.disable_pag()
    plain, _, _ = model(**call)
    model.enable_pag(pag_scale=PAG, pag_applied_layers=LAYERS)
    try:
        out, _, x0s = model(**call)
        zero, _, _ = model(pag_scale=0.0, **call)
    finally:
        model.disable_pag()
    assert len(x0s) == 3 and torch.equal(zero.images, plain.images)      # pag_scale = 0 is the plain call, bit for bit
    o = DDIMOracle()
    o.set_timesteps(3)
    ref = po.loop(sd, oracle_cfg(cfg), o, o.timesteps, pe, ne if cfg_on else None, lat, gs, LAYERS, PAG)
    _gate(f"DDIM 3 steps {PX} px cfg={cfg_on}", out.images, ref, plain.images)


def test_unipc_call_matches_the_oracle_loop(env):
    from tests.test_unipc_gpu import UniPCOracle
    cfg, sd, model = env
    lat, pe, ne = _inputs(cfg, 93)
    kw = dict(solver_order=2, solver_type="bh2")
    call = dict(prompt_embeds=pe, negative_prompt_embeds=ne, latents=lat, num_inference_steps=3, guidance_scale=GS, output_type="latent",
                height=PX, width=PX)
    _sched(model, "unipc_scheduler", **kw)
    plain, _, _ = model(**call)
    model.enable_pag(pag_scale=PAG, pag_applied_layers=LAYERS)
    try:
        _sched(model, "unipc_scheduler", **kw)
        out, _, _ = model(**call)
    finally:
        model.disable_pag()
    o = UniPCOracle(**kw)
    o.set_timesteps(3)
    ref = po.loop(sd, oracle_cfg(cfg), o, o.timesteps, pe, ne, lat, GS, LAYERS, PAG)
    _gate("UniPC 3 steps", out.images, ref, plain.images)


def test_image_to_image_call_matches_the_oracle_loop(env):
    """strength 0.6 of 5 DDIM steps: 3 run.  The oracle loop starts from the library's own noised encoding
    (tests/test_img2img_gpu.py holds the encoder to its oracle), so the gate sees the PAG loop alone."""
    from oracle.schedulers import DDIMOracle
    cfg, sd, model = env
    _, pe, ne = _inputs(cfg, 95)
    g = torch.Generator().manual_seed(96)
    img = torch.rand(1, 3, PX, PX, generator=g)
    call = dict(prompt_embeds=pe, negative_prompt_embeds=ne, image=img, strength=0.6, num_inference_steps=5, guidance_scale=GS,
                output_type="latent")
    _sched(model, "ddim_scheduler")
    plain, _, _ = model(generator=torch.Generator().manual_seed(97), **call)
    model.enable_pag(pag_scale=PAG, pag_applied_layers=LAYERS)
    try:
        out, _, x0s = model(generator=torch.Generator().manual_seed(97), **call)
    finally:
        model.disable_pag()
    t_start, steps = model.img2img_steps(5, 0.6)
    assert steps == 3 == len(x0s)
    start = model.img2img_start_latents.cpu()
    o = DDIMOracle()
    o.set_timesteps(5)
    ref = po.loop(sd, oracle_cfg(cfg), o, o.timesteps[t_start:], pe, ne, start, GS, LAYERS, PAG)
    _gate("img2img DDIM strength 0.6 of 5", out.images, ref, plain.images)


def test_adaptive_scale_reaching_zero_and_the_plan_count(env):
    """pag_adaptive_scale = 0.01 at scale 3: s_t = 0 from t = 700 down, so a 6-step DDIM run (t = 801, 668, ...) has one guided
    step and five at scale 0: finite images, another result than the plain call's.  Plain calls build no PAG plan."""
    from sonicdiffusionbayeslab_amd.schedulers import pag_step_scale
    cfg, sd, model = env
    lat, pe, ne = synth_inputs(cfg, 2, seed=99)
    call = dict(prompt_embeds=pe, negative_prompt_embeds=ne, latents=lat, num_inference_steps=6, guidance_scale=GS, output_type="latent")
    s = _sched(model, "ddim_scheduler")
    model.disable_pag()
    plain, _, _ = model(**call)
    plans = model.unet.plan_count()
    again, _, _ = model(**call)
    assert model.unet.plan_count() == plans and torch.equal(plain.images, again.images)
    model.enable_pag(pag_scale=PAG, pag_adaptive_scale=0.01, pag_applied_layers=LAYERS)
    try:
        zero, _, _ = model(pag_scale=0.0, **call)
        assert model.unet.plan_count() == plans and torch.equal(zero.images, plain.images)      # no PAG plan for a plain call
        out, _, _ = model(**call)
        assert model.unet.plan_count() > plans
        scales = [pag_step_scale(PAG, 0.01, t) for t in s._timesteps_list]
        assert scales[0] > 0.0 and scales.count(0.0) >= 4
        per_call, _, _ = model(pag_adaptive_scale=0.0, **call)          # the call's own value over enable_pag's
    finally:
        model.disable_pag()
    assert torch.isfinite(out.images).all() and not torch.equal(out.images, plain.images)
    assert torch.isfinite(per_call.images).all() and not torch.equal(per_call.images, out.images)
    plans = model.unet.plan_count()
    after, _, _ = model(**call)
    assert torch.equal(after.images, plain.images) and model.unet.plan_count() == plans
