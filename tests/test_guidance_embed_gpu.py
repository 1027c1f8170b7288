"""GPU parity of LCM-distilled UNets (diffusers ``time_cond_proj_dim``; reference src/models.py:195-202,231): the time
embedding adds ``cond_proj(get_guidance_scale_embedding(guidance_scale - 1))`` to the timestep sinusoid, CFG is off.

Operator level: the row GEMV and the sinusoid-plus-row kernel, every element against float64 with a-priori bounds
(tests/bounds.py), in guarded buffers.  UNet / loops: against the CPU oracle with the condition added by tests/cond_oracle.py,
under the tolerances of the plain path (UNET_TOL per forward as tests/test_unet_gpu.py, FREE_TOL / FREE_COS for free-running
loops as tests/test_pipeline_gpu.py, the lcm4 fixture's gate of tests/test_benchshapes_gpu.py for the 64x64 LCM loop, the fp8
loop gate of tests/test_fp8_gpu.py).  Without a condition the plan runs today's kernels: bit-identical to a plain handle."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from sonicdiffusionbayeslab_amd import _lib
from tests.bounds import ATOL_TINY, U32, assert_elementwise, check_guards, forget_guards, gemm_ref, guarded, guarded_input, \
    linear_bound, ulp_fp32
from tests.cond_oracle import COND, conditioned_oracle
from tests.util import cosine, oracle_cfg, rel_l2, synth_inputs

UNET_TOL = 2e-2                     # tests/test_unet_gpu.py
FREE_TOL, FREE_COS = 6e-2, 0.998    # tests/test_pipeline_gpu.py
LCM4_TOL, LCM4_COS = 1.5e-2, 0.999  # tests/test_benchshapes_gpu.py: LOOP_TOL["lcm4"]
FP8_FWD_TOL = 1.5e-1                # tests/test_fp8_gpu.py: FWD_TOL
D = 256
GUIDANCE = 8.0
DPM_KW = dict(solver_order=2, algorithm_type="dpmsolver++", final_sigmas_type="zero")

_KEEP = []


def stream():
    return torch.cuda.current_stream().cuda_stream


def P(t):
    _KEEP.append(t)
    return t.data_ptr()


@pytest.fixture(autouse=True)
def _drop_keep():
    yield
    torch.cuda.synchronize()
    _KEEP.clear()
    forget_guards()


def gemb(w, d=D):
    from sonicdiffusionbayeslab_amd.models import get_guidance_scale_embedding
    return get_guidance_scale_embedding(w, d)


# ---------------------------------------------------------------------------------------------------------------------
# operator level
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [256, 264, 8])
def test_row_gemv_and_sinusoid_plus_row(sdlib, d):
    g = torch.Generator().manual_seed(d)
    wc = (torch.randn(320, d, generator=g) / math.sqrt(d)).bfloat16().float()
    conds = [gemb(0.0, d)[0], gemb(7.0, d)[0], torch.randn(d, generator=g)]
    half = 160
    fd = torch.exp(-math.log(10000.0) * torch.arange(half, dtype=torch.float64) / half)
    for t in (981.0, 21.0):
        for ci, cond in enumerate(conds):
            row, emb = guarded((320,), torch.float32, label="row"), guarded((320,), torch.float32, label="emb")
            _lib.check(sdlib.sd_op_timestep_cond(stream(), t, P(guarded_input(cond, torch.float32, label="cond")),
                                                 P(guarded_input(wc, torch.bfloat16, label="W_cond")), P(row), P(emb), d, 320))
            torch.cuda.synchronize()
            check_guards()
            r, m = gemm_ref(cond[None], wc)
            assert_elementwise(row, r[0], linear_bound(r[0], m[0], d, torch.float32), f"cond_proj row d={d} cond {ci}")
            # sinusoid as tests/test_ops_gpu.py::test_time_embedding (<= 16 u |t f| of phase + 2^-21), then one rounding of
            # the addition of the kernel's own row
            row_k = row.double().cpu()
            ref = torch.cat([torch.cos(t * fd), torch.sin(t * fd)]) + row_k
            bound = 16 * U32 * t * torch.cat([fd, fd]) + 2.0 ** -21 + ulp_fp32(ref) + ATOL_TINY
            assert_elementwise(emb, ref, bound, f"sinusoid + row t={t} d={d} cond {ci}")


# ---------------------------------------------------------------------------------------------------------------------
# UNet level (16x16 latents, SD-1.5 widths)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small():
    from sonicdiffusionbayeslab_amd.unet import HipUNet2DConditionModel
    from sonicdiffusionbayeslab_amd.weights import UNetConfig, make_synthetic_state_dict
    cfg = UNetConfig(sample_size=16, time_cond_proj_dim=D)
    sd = make_synthetic_state_dict(cfg, seed=1234)
    net = HipUNet2DConditionModel(cfg, sd)
    pcfg = UNetConfig(sample_size=16)
    plain = HipUNet2DConditionModel(pcfg, {k: v for k, v in sd.items() if k != COND})
    return cfg, sd, net, plain


@pytest.mark.parametrize("t", [981.0, 21.0])
def test_conditioned_unet_forward_matches_oracle(small, t):
    from oracle.unet import unet_forward
    cfg, sd, net, _ = small
    lat, pe, _ = synth_inputs(cfg, 2)
    net.set_context(pe.cuda())
    eps = {}
    for w in (0.0, 7.0):
        with torch.no_grad(), conditioned_oracle(sd, w + 1.0):
            ref = unet_forward(sd, oracle_cfg(cfg), lat, t, pe)
        net.set_timestep_cond(gemb(w))
        eps[w] = net.forward_latents(lat.cuda(), 2, t).clone()
        torch.cuda.synchronize()
        err = rel_l2(eps[w], ref)
        print(f"conditioned forward t={t} w={w}: rel-L2 {err:.3e} cos {cosine(eps[w], ref):.5f}")
        assert torch.isfinite(eps[w]).all() and err < UNET_TOL
    net.set_timestep_cond(None)
    apart = rel_l2(eps[7.0], eps[0.0])
    print(f"w = 7 vs w = 0: rel-L2 {apart:.3e}")
    assert apart > 10 * UNET_TOL


def test_cleared_condition_is_the_plain_unet_bit_for_bit(small):
    cfg, sd, net, plain = small
    lat, pe, ne = synth_inputs(cfg, 2, seed=5)
    ctx = torch.cat([ne, pe]).cuda()
    for n in (net, plain):
        n.set_context(ctx)
    net.set_timestep_cond(gemb(7.0))
    cond = net.forward_latents(lat.cuda(), 4, 501.0).clone()
    net.set_timestep_cond(None)
    cleared = net.forward_latents(lat.cuda(), 4, 501.0).clone()
    ref = plain.forward_latents(lat.cuda(), 4, 501.0).clone()
    torch.cuda.synchronize()
    assert torch.equal(cleared, ref)
    assert rel_l2(cond, ref) > 10 * UNET_TOL
    # the condition lives in the handle: it survives DeepCache plans and other sizes, and costs no launch per forward
    net.set_timestep_cond(gemb(7.0))
    prof_c = net.forward_profiled(lat.cuda(), 4, 501.0)
    prof_p = plain.forward_profiled(lat.cuda(), 4, 501.0)
    assert {k: v["launches"] for k, v in prof_c.items()} == {k: v["launches"] for k, v in prof_p.items()}
    net.set_deepcache(0)
    net.set_context(ctx)
    branch = net.forward_latents(lat.cuda(), 4, 501.0).clone()
    net.set_timestep_cond(None)
    branch_plain = net.forward_latents(lat.cuda(), 4, 501.0).clone()
    net.set_deepcache(-1)
    torch.cuda.synchronize()
    assert rel_l2(branch, cond) < UNET_TOL / 4 and rel_l2(branch_plain, ref) < UNET_TOL / 4
    assert rel_l2(branch, branch_plain) > 10 * UNET_TOL


def test_diffusers_style_call_with_timestep_cond(small):
    cfg, sd, net, plain = small
    lat, pe, _ = synth_inputs(cfg, 2, seed=3)
    ctx, x = pe.cuda(), lat.cuda()
    tc = gemb(7.0).repeat(2, 1)
    a = net(x, torch.tensor(501), encoder_hidden_states=ctx, timestep_cond=tc, return_dict=False)[0].clone()
    b1 = net(x, 501, encoder_hidden_states=ctx, timestep_cond=tc[0])[0].clone()
    net.set_timestep_cond(gemb(7.0))
    net.set_context(ctx)
    b = net.forward_latents(lat.cuda(), 2, 501.0).clone()
    none = net(x, 501, encoder_hidden_states=ctx)[0].clone()            # timestep_cond=None: no projection (diffusers)
    p = plain(x, 501, encoder_hidden_states=ctx)[0]
    torch.cuda.synchronize()
    assert torch.equal(a, b) and torch.equal(b1, b) and torch.equal(none, p)
    bad = tc.clone()
    bad[1] = gemb(3.0)[0]
    with pytest.raises(ValueError, match="one row"):
        net(x, 501, encoder_hidden_states=ctx, timestep_cond=bad)
    with pytest.raises(ValueError, match="cond_proj"):
        plain(x, 501, encoder_hidden_states=ctx, timestep_cond=tc)
    with pytest.raises(NotImplementedError):
        net(x, 501, encoder_hidden_states=ctx, added_cond_kwargs={})
    net.set_timestep_cond(None)


# ---------------------------------------------------------------------------------------------------------------------
# loops, all at guidance_scale 8 (w = 7)
# ---------------------------------------------------------------------------------------------------------------------
def _load_lcm_cond_golden():
    import importlib.util
    import os

    import numpy as np
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    spec = importlib.util.spec_from_file_location("make_lcm_cond_golden", os.path.join(here, "make_lcm_cond_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod, np.load(os.path.join(here, "lcm_cond_golden_64.npz"))


@pytest.fixture(scope="module")
def full():
    """The full-size (64x64) conditioned pipeline of the fixture."""
    from sonicdiffusionbayeslab_amd.models import StableDiffusionModel
    from sonicdiffusionbayeslab_amd.weights import make_synthetic_state_dict
    mod, z = _load_lcm_cond_golden()
    cfg = mod.config()
    sd = make_synthetic_state_dict(cfg, seed=mod.WEIGHTS_SEED)
    assert str(z["weights_fingerprint"]) == mod.weights_fingerprint(sd), "fixture was generated for other synthetic weights"
    model = StableDiffusionModel(unet_config=cfg, state_dict=dict(sd)).to("cuda:0")
    return mod, z, cfg, sd, model


def _sched(name, **kw):
    from sonicdiffusionbayeslab_amd.registry import schedulers_registry
    from sonicdiffusionbayeslab_amd.schedulers import PNDMConfigStub
    return schedulers_registry[name].from_config(PNDMConfigStub().config, **kw)


def test_lcm4_guidance_conditioned_at_64x64_against_the_oracle_fixture(full):
    mod, z, cfg, sd, model = full
    model.scheduler = _sched("lcm_scheduler")
    lat, pe, noise = mod.inputs(cfg)
    assert mod.digest(lat) == str(z["init_sha256"]) and mod.digest(noise) == str(z["noise_sha256"])
    assert float(z["guidance_scale"]) == GUIDANCE
    out, secs, _ = model(prompt_embeds=pe, latents=lat, num_inference_steps=4, guidance_scale=GUIDANCE, output_type="latent",
                         step_noise=noise.cuda())
    assert not model.do_classifier_free_guidance
    got, ref = out.images.float().cpu(), torch.as_tensor(z["step4"]).float()
    rl, cs = rel_l2(got, ref), cosine(got, ref)
    print(f"LCM 4 steps, guidance-conditioned, 64x64 batch 2 vs the oracle fixture: rel-L2 {rl:.3e} cos {cs:.5f}, "
          f"loop {secs * 1e3:.1f} ms")
    assert rl < LCM4_TOL and cs > LCM4_COS


def test_one_512x768_conditioned_forward(full):
    from oracle.unet import unet_forward
    mod, z, cfg, sd, model = full
    net = model.unet
    g = torch.Generator().manual_seed(61)
    lat = torch.randn(1, 4, 64, 96, generator=g)
    pe = torch.randn(1, 77, 768, generator=g)
    net.set_deepcache(-1)
    net.set_context(pe.cuda(), 64, 96)
    net.set_timestep_cond(gemb(GUIDANCE - 1.0))
    eps = net.forward_latents(lat.cuda(), 1, 499.0)
    torch.cuda.synchronize()
    with torch.no_grad(), conditioned_oracle(sd, GUIDANCE):
        ref = unet_forward(sd, oracle_cfg(cfg), lat, 499.0, pe)
    err = rel_l2(eps, ref)
    print(f"512x768 conditioned forward: rel-L2 {err:.3e} cos {cosine(eps, ref):.5f}")
    assert torch.isfinite(eps).all() and err < UNET_TOL


@pytest.fixture(scope="module")
def small_cfg():
    from sonicdiffusionbayeslab_amd.weights import UNetConfig, make_synthetic_state_dict
    cfg = UNetConfig(sample_size=16, time_cond_proj_dim=D)
    return cfg, make_synthetic_state_dict(cfg, seed=1234)


def _model(small_cfg, key="stable_diffusion_model", **kw):
    from sonicdiffusionbayeslab_amd.registry import models_registry
    cfg, sd = small_cfg
    return models_registry[key](unet_config=cfg, state_dict=dict(sd), **kw).to("cuda:0")


def test_deepcache_interval_2_conditioned(small_cfg):
    from oracle.pipeline import sample_loop
    from oracle.schedulers import DDIMOracle
    from oracle.unet import DeepCacheState
    from sonicdiffusionbayeslab_amd.deepcache import DeepCacheSDHelper
    cfg, sd = small_cfg
    model = _model(small_cfg)
    model.scheduler = _sched("ddim_scheduler")
    lat, pe, _ = synth_inputs(cfg, 2, seed=41)
    helper = DeepCacheSDHelper(pipe=model)
    helper.set_params(cache_interval=2, cache_branch_id=0)
    helper.enable()
    try:
        out, _, _ = model(prompt_embeds=pe, latents=lat, num_inference_steps=6, guidance_scale=GUIDANCE, output_type="latent")
    finally:
        helper.disable()
    dc = DeepCacheState(cache_interval=2, cache_branch_id=0, enabled=True)
    with conditioned_oracle(sd, GUIDANCE):
        ref, _, _, _ = sample_loop(sd, oracle_cfg(cfg), DDIMOracle(), pe, None, lat, 6, 1.0, deepcache=dc)
    err, cs = rel_l2(out.images, ref), cosine(out.images, ref)
    print(f"DeepCache N=2 branch 0, conditioned DDIM 6 steps: rel-L2 {err:.3e} cos {cs:.5f}")
    assert err < FREE_TOL and cs > FREE_COS


def test_variant_pipelines_two_steps_conditioned(small_cfg):
    from oracle.pipeline import sample_loop_interleaving, sample_loop_skip, sample_loop_two_schedulers
    from oracle.schedulers import DDIMOracle, DPMSolverOracle
    cfg, sd = small_cfg
    lat, pe, _ = synth_inputs(cfg, 1, seed=43)
    ocfg = oracle_cfg(cfg)
    runs = []
    m = _model(small_cfg, "stable_diffusion_model_two_schedulers")
    m.scheduler_first, m.scheduler_second = _sched("ddim_scheduler"), _sched("dpm_solver_scheduler", **DPM_KW)
    out, _, _ = m(prompt_embeds=pe, latents=lat, guidance_scale=GUIDANCE, num_inference_steps_first=2,
                  num_inference_steps_second=2, num_step_switch=1, type_switch="closest", output_type="latent")
    with conditioned_oracle(sd, GUIDANCE):
        ref, _, used = sample_loop_two_schedulers(sd, ocfg, DDIMOracle(), DPMSolverOracle(**DPM_KW), pe, None, lat, 2, 1,
                                                  "closest", 1.0)
    runs.append(("two schedulers", out.images, ref, len(used)))
    del m
    m = _model(small_cfg, "stable_diffusion_model_interliving_schedulers")
    m.scheduler_main, m.scheduler_inter = _sched("dpm_solver_scheduler", **DPM_KW), _sched("ddim_scheduler")
    out, _, _ = m(prompt_embeds=pe, latents=lat, guidance_scale=GUIDANCE, num_inference_steps=3, interliving_steps=[0],
                  output_type="latent")
    with conditioned_oracle(sd, GUIDANCE):
        ref, _, keep = sample_loop_interleaving(sd, ocfg, DPMSolverOracle(**DPM_KW), DDIMOracle(), pe, None, lat, 3, [0], 1.0)
    runs.append(("interleaved", out.images, ref, len(keep)))
    del m
    m = _model(small_cfg, "stable_diffusion_model_skip_timesteps")
    m.scheduler = _sched("ddim_scheduler")
    out, _, _ = m(prompt_embeds=pe, latents=lat, guidance_scale=GUIDANCE, num_inference_steps=3, skip_timesteps=[1],
                  output_type="latent")
    with conditioned_oracle(sd, GUIDANCE):
        ref, _, used = sample_loop_skip(sd, ocfg, DDIMOracle(), pe, None, lat, 3, [1], 1.0)
    runs.append(("skip", out.images, ref, len(used)))
    del m
    for name, got, ref, n in runs:
        err, cs = rel_l2(got, ref), cosine(got, ref)
        print(f"{name} ({n} steps), conditioned: rel-L2 {err:.3e} cos {cs:.5f}")
        assert err < FREE_TOL and cs > FREE_COS


def test_fp8_calibration_is_independent_of_the_call_guidance_and_the_loop_matches(small_cfg):
    from oracle.fp8 import Fp8Emulation
    from oracle.pipeline import sample_loop
    from oracle.schedulers import LCMOracle
    cfg, sd = small_cfg
    lat, pe, _ = synth_inputs(cfg, 2, seed=17)
    noise = torch.randn(1, 2, 4, 16, 16, generator=torch.Generator().manual_seed(8))
    a = _model(small_cfg, weight_dtype="fp8")
    a.scheduler = _sched("lcm_scheduler")
    out, _, _ = a(prompt_embeds=pe, latents=lat, num_inference_steps=2, guidance_scale=GUIDANCE, output_type="latent",
                  step_noise=noise.cuda())
    scales_a = dict(a.fp8_scales)
    assert scales_a and "calibrated" in a.weights_source
    del a
    b = _model(small_cfg, weight_dtype="fp8")
    b.scheduler = _sched("lcm_scheduler")
    b(prompt_embeds=pe[:1], latents=lat[:1], num_inference_steps=1, guidance_scale=2.0, output_type="latent")
    assert dict(b.fp8_scales) == scales_a          # the fixed calibration guidance, not the call's
    del b
    with conditioned_oracle(sd, GUIDANCE):
        ref_q, _, _, _ = sample_loop(sd, oracle_cfg(cfg), LCMOracle(), pe, None, lat, 2, 0.0, lcm_noise=noise,
                                     fq=Fp8Emulation(sd, scales=scales_a))
    e_q, cs = rel_l2(out.images, ref_q), cosine(out.images, ref_q)
    print(f"LCM 2 steps fp8, conditioned: vs emulating oracle {e_q:.3e} cos {cs:.5f}")
    assert e_q < FP8_FWD_TOL and cs > 0.99
