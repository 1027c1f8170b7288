"""Rescaled CFG (guidance_rescale), v-prediction and zero-terminal-SNR schedules on the GPU.

Kernel level: sd_cfg_rescale_factors + sd_sched_step_rescaled against the fp64 restatement (tests/sched_ref.py), per
element, with every operand and output between guard bands (tests/bounds.py) and an a-priori bound; the factor of a sample
must be bit-identical whatever batch it is computed in and wherever it sits.  Scheduler level: full teacher-forced
trajectories on random model outputs.  Pipeline level: the synthetic 16x16 UNet against the oracle UNet driven by the
restated scheduler, with the free-running gates of test_pipeline_gpu.py."""
import ctypes as C
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import bounds as BD
from tests import sched_ref as R
from tests.util import cosine, oracle_cfg, rel_l2, synth_inputs

U = 2.0 ** -24
FREE_TOL, FREE_COS = 6e-2, 0.998
SIZES = [(16, 16), (32, 32), (40, 56), (64, 64), (128, 128)]


def _factors(lib, eps, B, n, s, r, k):
    from sonicdiffusionbayeslab_amd import _lib
    _lib.check(lib.sd_cfg_rescale_factors(_lib.current_stream(), eps.data_ptr(), B, n, s, r, k.data_ptr()))


def _step(lib, eps, s, x, ms, z, prev, y2, mo, coef, k, n_per):
    from sonicdiffusionbayeslab_amd import _lib
    carr = (C.c_float * 10)(*[float(v) for v in coef])
    _lib.check(lib.sd_sched_step_rescaled(_lib.current_stream(), eps.data_ptr(), 1, s, x.data_ptr(), ms[0].data_ptr(),
                                          ms[1].data_ptr(), ms[2].data_ptr(), z.data_ptr(), prev.data_ptr(), y2.data_ptr(),
                                          mo.data_ptr(), carr, x.numel(), k.data_ptr(), n_per))


def _inputs(B, h, w, seed):
    g = torch.Generator().manual_seed(seed)
    e2 = torch.randn(2 * B, 4, h, w, generator=g)
    e2[B:] = 1.7 * e2[B:] + 0.3                      # text half: another scale and mean than the uncond half
    ops = [torch.randn(B, 4, h, w, generator=g) for _ in range(5)]   # x, m1, m2, m3, noise
    coef = (torch.rand(10, generator=g) * 2 - 1).tolist()
    return e2, ops, [float(torch.tensor(c, dtype=torch.float32)) for c in coef]


def _run(lib, e2, ops, coef, s, r):
    B, n = ops[0].shape[0], ops[0][0].numel()
    eps = BD.guarded_input(e2, label="eps")
    x, m1, m2, m3, z = (BD.guarded_input(t, label=l) for t, l in zip(ops, ("x", "m1", "m2", "m3", "noise")))
    k = BD.guarded((B,), torch.float32, label="k")
    prev, y2, mo = (BD.guarded(tuple(ops[0].shape), torch.float32, label=l) for l in ("prev", "y2", "m_out"))
    _factors(lib, eps, B, n, s, r, k)
    _step(lib, eps, s, x, (m1, m2, m3), z, prev, y2, mo, coef, k, n)
    torch.cuda.synchronize()
    out = [t.cpu().clone() for t in (k, prev, y2, mo)]
    BD.check_guards()
    return out


def _reference(e2, ops, coef, s, r):
    """fp64 k, prev, y2, m_out and their a-priori bounds."""
    B = ops[0].shape[0]
    u, c = e2.double().chunk(2)
    g = R.cfg_combine(u, c, s)
    k = R.rescale_factor(g, c, r).flatten()
    kk = k.view(-1, 1, 1, 1)
    e = kk * g
    # g in fp32: (c - u), s * (.), + u -- at most three roundings, each <= u |its result|
    Eg = U * (2.0 * abs(s) * (c - u).abs() + g.abs()) * (1 + 1e-6)
    dims = (1, 2, 3)
    gc = g - g.mean(dim=dims, keepdim=True)
    ds = Eg.pow(2).sum(dim=dims).sqrt() / gc.pow(2).sum(dim=dims).sqrt() + 1e-12      # rel. error of std(g)
    ratio = (k - (1.0 - r)) / r if r > 0 else torch.zeros_like(k)
    Bk = r * ratio * (ds / (1 - ds)) * 1.01 + BD.ulp_fp32(k)
    Ee = ((kk.abs() + Bk.view(-1, 1, 1, 1)) * Eg + g.abs() * Bk.view(-1, 1, 1, 1) + U * e.abs()) * 1.01
    x, m1, m2, m3, z = (t.double() for t in ops)
    px, pe, p1, p2, pn, yx, ye, mx, me, p3 = coef
    prev = px * x + pe * e + p1 * m1 + p2 * m2 + p3 * m3 + pn * z
    pmag = abs(px) * x.abs() + abs(pe) * e.abs() + abs(p1) * m1.abs() + abs(p2) * m2.abs() + abs(p3) * m3.abs() + abs(pn) * z.abs()
    y2 = yx * x + ye * e
    mo = mx * x + me * e
    out = [(k, Bk),
           (prev, BD.linear_bound(prev, pmag, 6, out=torch.float32) + abs(pe) * Ee),
           (y2, BD.linear_bound(y2, abs(yx) * x.abs() + abs(ye) * e.abs(), 2, out=torch.float32) + abs(ye) * Ee),
           (mo, BD.linear_bound(mo, abs(mx) * x.abs() + abs(me) * e.abs(), 2, out=torch.float32) + abs(me) * Ee)]
    return out


WORST = {}


@pytest.mark.parametrize("r", [0.3, 0.7, 1.0])
@pytest.mark.parametrize("B", [1, 2, 7, 8])
@pytest.mark.parametrize("hw", SIZES, ids=[f"{h}x{w}" for h, w in SIZES])
def test_rescale_kernels_elementwise(sdlib, hw, B, r):
    h, w = hw
    e2, ops, coef = _inputs(B, h, w, seed=h * 1000 + w + B)
    got = _run(sdlib, e2, ops, coef, 7.5, r)
    for name, g, (ref, bound) in zip(("k", "prev", "y2", "m_out"), got, _reference(e2, ops, coef, 7.5, r)):
        ratio = BD.assert_elementwise(g, ref, bound, f"{name} {h}x{w} B={B} r={r}")
        WORST[name] = max(WORST.get(name, 0.0), ratio)
    print("worst error / bound so far:", {k: f"{v:.3f}" for k, v in WORST.items()})


@pytest.mark.parametrize("hw", [(16, 16), (40, 56), (64, 64), (128, 128)], ids=lambda t: f"{t[0]}x{t[1]}")
def test_rescale_batch_invariance(sdlib, hw):
    """A sample's factor and step outputs are bit-identical alone, at another position and in a batch of 8."""
    h, w = hw
    e2, ops, coef = _inputs(8, h, w, seed=77)
    full = _run(sdlib, e2, ops, coef, 7.5, 0.7)
    for b in (0, 3, 7):
        alone = _run(sdlib, torch.cat([e2[b:b + 1], e2[8 + b:9 + b]]), [t[b:b + 1] for t in ops], coef, 7.5, 0.7)
        for a, f in zip(alone, full):
            assert torch.equal(a, f[b:b + 1]), b
        # sample b at position 1 of a batch of 3 (its neighbours are other samples)
        o = [(b + 1) % 8, b, (b + 5) % 8]
        moved = _run(sdlib, torch.cat([e2[o], e2[[8 + j for j in o]]]), [t[o] for t in ops], coef, 7.5, 0.7)
        for a, f in zip(moved, full):
            assert torch.equal(a[1:2], f[b:b + 1]), b


def test_rescale_argument_checks(sdlib):
    from sonicdiffusionbayeslab_amd import _lib
    eps = torch.zeros(2, 4, 4, 4, device="cuda")
    k = torch.zeros(1, device="cuda")
    assert sdlib.sd_cfg_rescale_factors(_lib.current_stream(), eps.data_ptr(), 1, 6, 7.5, 0.7, k.data_ptr()) != 0
    assert sdlib.sd_cfg_rescale_factors(_lib.current_stream(), eps.data_ptr(), 0, 64, 7.5, 0.7, k.data_ptr()) != 0
    assert sdlib.sd_cfg_rescale_factors(_lib.current_stream(), None, 1, 64, 7.5, 0.7, k.data_ptr()) != 0


# ------------------------------------------------------------------------------------------------ scheduler level
TRAJ = [("ddim", dict(timestep_spacing="trailing"), 10, True),
        ("dpm", dict(solver_order=2, algorithm_type="dpmsolver++", timestep_spacing="trailing"), 10, True),
        ("dpm", dict(solver_order=2, algorithm_type="sde-dpmsolver++", timestep_spacing="trailing"), 10, True),
        ("lcm", {}, 4, True),
        ("pndm", {}, 8, False)]


@pytest.mark.parametrize("r", [0.0, 0.7])
@pytest.mark.parametrize("kind,kw,n,zsnr", TRAJ, ids=[f"{t[0]}-{t[1].get('algorithm_type', '')}-{t[2]}" for t in TRAJ])
def test_scheduler_trajectories_match_restatement(kind, kw, n, zsnr, r):
    """v-prediction (and zero SNR where the scheduler takes it) over a full schedule, teacher-forced per step."""
    s, ref = R.make_pair(kind, n, "v_prediction", zsnr, **kw)
    if zsnr and kind != "dpm":
        assert s.alphas_cumprod[s._timesteps_list[0]] == 0.0           # the schedule starts at zero SNR
    worst = [0.0]

    def check(i, got, want):
        for a, b in zip(got, want):
            e = rel_l2(a, b)
            worst[0] = max(worst[0], e)
            assert e < 1e-5, (i, e)
            assert (a.double().cpu() - b).abs().max().item() <= 1e-5 * (b.abs().max().item() + 1.0), i
        if r > 0:
            assert s.rescale_factors is not None and s.rescale_factors.shape == (2,)
        else:
            assert s.rescale_factors is None

    R.run_teacher_forced(s, ref, kind, (2, 4, 16, 16), 7.5, r, "cuda", check)
    print(f"{kind} {kw} v zsnr={zsnr} r={r}: worst rel-L2 {worst[0]:.2e}")


# ------------------------------------------------------------------------------------------------ pipeline level
@pytest.fixture(scope="module")
def env():
    from sonicdiffusionbayeslab_amd.weights import UNetConfig, make_synthetic_state_dict
    cfg = UNetConfig(sample_size=16)
    return cfg, make_synthetic_state_dict(cfg, seed=1234)


VZ = dict(prediction_type="v_prediction", rescale_betas_zero_snr=True, timestep_spacing="trailing")
DPM_KW = dict(solver_order=2, algorithm_type="dpmsolver++", final_sigmas_type="zero")


def _sched(name, **kw):
    from sonicdiffusionbayeslab_amd.registry import schedulers_registry
    from sonicdiffusionbayeslab_amd.schedulers import PNDMConfigStub
    return schedulers_registry[name].from_config(PNDMConfigStub().config, **kw)


def _ref_ddim(n):
    s = _sched("ddim_scheduler", **VZ)
    s.set_timesteps(n)
    return R.DDIM(torch.from_numpy(s.alphas_cumprod), s._timesteps_list, "v_prediction", s.final_alpha_cumprod), \
        s._timesteps_list


@torch.no_grad()
def _ref_loop(sd, cfg, pe, ne, lat, plan, gs, r):
    """plan: [(scheduler restatement, t, hand-off target or None)]"""
    from oracle.unet import unet_forward
    ocfg = oracle_cfg(cfg)
    ctx = torch.cat([ne, pe])
    x = lat.double()
    for sched, t, other in plan:
        xin = x.float()
        m = R.guided(unet_forward(sd, ocfg, torch.cat([xin, xin]), t, ctx), gs, r)
        x = sched.step(m, t, x)[0]
        if other is not None:
            other.push(m, x)
    return x


def test_call_v_prediction_zero_snr_rescaled(env):
    from sonicdiffusionbayeslab_amd.models import StableDiffusionModel
    cfg, sd = env
    model = StableDiffusionModel(unet_config=cfg, state_dict=dict(sd)).to("cuda:0")
    model.scheduler = _sched("ddim_scheduler", **VZ)
    lat, pe, ne = synth_inputs(cfg, 2, seed=53)
    n = 6
    out, _, x0s = model(prompt_embeds=pe, negative_prompt_embeds=ne, latents=lat, num_inference_steps=n,
                        guidance_scale=7.5, guidance_rescale=0.7, output_type="latent")
    assert model.scheduler.rescale_factors is not None and len(x0s) == n
    ref_s, ts = _ref_ddim(n)
    ref = _ref_loop(sd, cfg, pe, ne, lat, [(ref_s, t, None) for t in ts], 7.5, 0.7)
    err, cs = rel_l2(out.images, ref), cosine(out.images, ref)
    plain = _ref_loop(sd, cfg, pe, ne, lat, [(_ref_ddim(n)[0], t, None) for t in ts], 7.5, 0.0)
    print(f"DDIM v / zero SNR / trailing, guidance_rescale 0.7, {n} steps: rel-L2 {err:.3e} cos {cs:.5f}; "
          f"reference with vs without the rescale: rel-L2 {rel_l2(ref, plain):.3e}")
    assert err < FREE_TOL and cs > FREE_COS
    assert rel_l2(out.images, plain) > 3 * err          # the rescale is visible beyond the loop's own error


def test_two_schedulers_rescaled_hand_off(env):
    from oracle.pipeline import switch_timestamp
    from sonicdiffusionbayeslab_amd.registry import models_registry
    cfg, sd = env
    model = models_registry["stable_diffusion_model_two_schedulers"](unet_config=cfg, state_dict=dict(sd)).to("cuda:0")
    model.scheduler_first = _sched("ddim_scheduler", **VZ)
    model.scheduler_second = _sched("dpm_solver_scheduler", **VZ, **DPM_KW)
    lat, pe, ne = synth_inputs(cfg, 1, seed=59)
    n_first, switch = 8, 3
    out, _, _ = model(prompt_embeds=pe, negative_prompt_embeds=ne, latents=lat, guidance_scale=7.5,
                      num_inference_steps_first=n_first, num_inference_steps_second=n_first, num_step_switch=switch,
                      type_switch="closest", guidance_rescale=0.7, output_type="latent")
    first_s, ts = _ref_ddim(n_first)
    d = _sched("dpm_solver_scheduler", **VZ, **DPM_KW)
    d.set_timesteps(timesteps=ts)
    second_s = R.DPM(torch.from_numpy(d.alphas_cumprod), ts, "v_prediction", **DPM_KW)
    first, second = switch_timestamp(ts, ts, switch, "closest")
    plan = [(first_s, t, second_s) for t in first] + [(second_s, t, None) for t in second]
    ref = _ref_loop(sd, cfg, pe, ne, lat, plan, 7.5, 0.7)
    err, cs = rel_l2(out.images, ref), cosine(out.images, ref)
    print(f"two schedulers (DDIM -> DPM++ 2, v / zero SNR), guidance_rescale 0.7: rel-L2 {err:.3e} cos {cs:.5f}")
    assert model.num_timesteps == len(plan)
    assert err < FREE_TOL and cs > FREE_COS


def test_guidance_rescale_zero_is_the_default_path(env):
    from sonicdiffusionbayeslab_amd.models import StableDiffusionModel
    cfg, sd = env
    model = StableDiffusionModel(unet_config=cfg, state_dict=dict(sd)).to("cuda:0")
    lat, pe, ne = synth_inputs(cfg, 2, seed=61)
    outs = []
    for kw in ({}, {"guidance_rescale": 0.0}):
        model.scheduler = _sched("ddim_scheduler")
        outs.append(model(prompt_embeds=pe, negative_prompt_embeds=ne, latents=lat, num_inference_steps=4,
                          guidance_scale=7.5, output_type="latent", **kw)[0].images)
    assert torch.equal(outs[0], outs[1])
