"""GPU parity of inpainting: the three new kernels per element (bit-exact where the arithmetic allows it, a-priori bounds
elsewhere, guard bands round every operand), whole inpainting loops against the restated loop (tests/inpaint_oracle.py) at
the free-running gates of tests/test_pipeline_gpu.py, and the exact properties of the 4-channel blend."""
import ctypes as C
import dataclasses
import json

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from sonicdiffusionbayeslab_amd import _lib
from tests.bounds import (ATOL_TINY, NHWC, U32, assert_elementwise, check_guards, conv3x3_nhwc_ref, forget_guards, guarded,
                          guarded_input, linear_bound)
from tests.util import cosine, oracle_cfg, rel_l2, synth_inputs

ENC_TOL, ENC_COS = 2e-2, 0.999            # the encoder's gates (tests/test_img2img_gpu.py): start and image latents
FREE_TOL, FREE_COS = 6e-2, 0.998          # tests/test_pipeline_gpu.py: final latents of a free-running loop


def stream():
    return torch.cuda.current_stream().cuda_stream


@pytest.fixture(autouse=True)
def _drop_guards():
    yield
    torch.cuda.synchronize()
    forget_guards()


def bits(t):
    return t.contiguous().view(torch.int32)


# ---------------------------------------------------------------- sd_inpaint_prepare
@pytest.mark.parametrize("B,H,W", [(2, 24, 40), (1, 128, 128)])
def test_inpaint_prepare_is_bit_exact(sdlib, B, H, W):
    g = torch.Generator().manual_seed(100 + H)
    img = torch.rand(B, 3, H, W, generator=g)
    m = torch.rand(B, 1, H, W, generator=g)                       # another pattern for every sample
    below = float(torch.nextafter(torch.tensor(0.5), torch.tensor(0.0)))
    m[:, 0, 0, :4] = torch.tensor([0.5, below, 0.0, 1.0])         # (0, 0) is a latent-mask pixel: exactly 0.5 -> repaint
    m[:, 0, 8, 8:12] = torch.tensor([below, 0.5, 1.0, 0.0])       # (8, 8) too: just below 0.5 -> keep
    m[B - 1, 0, 16, 16] = 0.5
    imgd, md = guarded_input(img), guarded_input(m)
    masked, lmask = guarded((B, 3, H, W), torch.float32), guarded((B, 1, H // 8, W // 8), torch.float32)
    _lib.check(sdlib.sd_inpaint_prepare(stream(), imgd.data_ptr(), md.data_ptr(), masked.data_ptr(), lmask.data_ptr(), B, H, W))
    torch.cuda.synchronize()
    check_guards()
    want = torch.where(m >= .5, .5, img)
    want_l = (m[..., ::8, ::8] >= .5).float()
    assert torch.equal(bits(masked.cpu()), bits(want))
    assert torch.equal(bits(lmask.cpu()), bits(want_l))
    assert want_l[0, 0, 0, 0] == 1.0 and want_l[0, 0, 1, 1] == 0.0 and 0.0 < float(want_l.mean()) < 1.0


# ---------------------------------------------------------------- sd_sched_step_inpaint
STEP_B, STEP_C, STEP_H, STEP_W = 3, 4, 8, 24          # 3 * 4 * 192 / 4 = 576 vectors: two full blocks and a tail of 64
COEF = (0.93, -0.41, 0.27, -0.13, 0.35, 1.07, -0.52, 0.88, -0.61, 0.0)


def _step_operands(cfg, seed):
    g = torch.Generator().manual_seed(seed)
    shp = (STEP_B, STEP_C, STEP_H, STEP_W)
    t = {n: torch.randn(shp, generator=g) for n in ("x", "m1", "m2", "noise", "init", "bnoise")}
    t["eps"] = torch.randn(((2 if cfg else 1) * STEP_B,) + shp[1:], generator=g)
    t["k"] = 0.6 + 0.5 * torch.rand(STEP_B, generator=g)
    mask = (torch.rand(STEP_B, 1, STEP_H, STEP_W, generator=g) > 0.5).float()      # per sample, varying along both axes
    assert all(0 < int(mask[b].sum()) < STEP_H * STEP_W for b in range(STEP_B))
    assert not torch.equal(mask[0], mask[1]) and not torch.equal(mask[1], mask[2])
    assert (mask != mask[:, :, :1]).any() and (mask != mask[:, :, :, :1]).any()
    t["mask"] = mask
    return t


def _run_step(sdlib, t, cfg, use_k, blend):
    """One launch on guarded operands.  blend = None: sd_sched_step / sd_sched_step_rescaled; (a, s): sd_sched_step_inpaint."""
    d = {n: guarded_input(v) for n, v in t.items()}
    shp = (STEP_B, STEP_C, STEP_H, STEP_W)
    prev, y2, mo = (guarded(shp, torch.float32) for _ in range(3))
    carr = (C.c_float * 10)(*COEF)
    n, nps, gs = t["x"].numel(), STEP_C * STEP_H * STEP_W, 7.5
    head = (stream(), d["eps"].data_ptr(), int(cfg), gs, d["x"].data_ptr(), d["m1"].data_ptr(), d["m2"].data_ptr(), None,
            d["noise"].data_ptr(), prev.data_ptr(), y2.data_ptr(), mo.data_ptr(), carr, n)
    if blend is not None:
        _lib.check(sdlib.sd_sched_step_inpaint(*head, d["k"].data_ptr() if use_k else None, nps, d["init"].data_ptr(),
                                               d["bnoise"].data_ptr(), d["mask"].data_ptr(), blend[0], blend[1],
                                               STEP_H * STEP_W))
    elif use_k:
        _lib.check(sdlib.sd_sched_step_rescaled(*head, d["k"].data_ptr(), nps))
    else:
        _lib.check(sdlib.sd_sched_step(*head))
    torch.cuda.synchronize()
    check_guards()
    return prev.cpu(), y2.cpu(), mo.cpu()


@pytest.mark.parametrize("cfg", [False, True])
@pytest.mark.parametrize("use_k", [False, True])
def test_sched_step_inpaint_per_element(sdlib, cfg, use_k):
    """Where the mask is 1: the bits of the unmasked kernel.  Where it is 0: a * init + s * blend_noise, two rounded products
    and one rounded sum (or a product and an fma, which is no worse) -> |err| <= 2 U (|a init| + |s noise|) to first order,
    with 1 % for the second-order terms.  y2 and m_out: the unmasked kernel's bits everywhere."""
    t = _step_operands(cfg, seed=7 + 2 * cfg + use_k)
    a, s = 0.8125 + 2.0 ** -12, 0.58203125 + 2.0 ** -13
    a32, s32 = float(torch.tensor(a, dtype=torch.float32)), float(torch.tensor(s, dtype=torch.float32))
    p0, y0, m0 = _run_step(sdlib, t, cfg, use_k, None)
    p1, y1, m1 = _run_step(sdlib, t, cfg, use_k, (a, s))
    rep = (t["mask"] >= 0.5).expand_as(p0)
    assert torch.equal(bits(y1), bits(y0)) and torch.equal(bits(m1), bits(m0))
    assert torch.equal(bits(p1)[rep], bits(p0)[rep])
    ai, sn = a32 * t["init"].double(), s32 * t["bnoise"].double()
    bound = 1.01 * 2 * U32 * (ai.abs() + sn.abs()) + ATOL_TINY
    ref = torch.where(rep, p1.double(), ai + sn)              # (the step side was compared bit for bit above)
    assert_elementwise(p1, ref, bound, f"sched_step_inpaint kept side cfg={cfg} k={use_k}", ("b", "c", "y", "x"))
    assert (p1[~rep] != p0[~rep]).any()
    # (a, s) = (1, 0): the kept side is init, bit for bit; the step side is untouched
    p2, y2, m2 = _run_step(sdlib, t, cfg, use_k, (1.0, 0.0))
    assert torch.equal(bits(p2)[~rep], bits(t["init"])[~rep]) and torch.equal(bits(p2)[rep], bits(p0)[rep])
    assert torch.equal(bits(y2), bits(y0)) and torch.equal(bits(m2), bits(m0))


# ---------------------------------------------------------------- sd_op_conv_in_cond
@pytest.mark.parametrize("H,W", [(8, 8), (10, 22)])
@pytest.mark.parametrize("Cout", [320, 64])
def test_conv_in_cond_per_element(sdlib, H, W, Cout):
    """B = 4 from source batches of 2 (CFG duplication).  Against fp64 F.conv2d of the concatenated input: fp32 inputs and
    weights, so 81 rounded products, 81 additions and the bias -> linear_bound(k_eff = 2 * 81 + 1), the 4-channel test's
    counting.  With zero weights on the five condition channels the kernel guarantees the 4-channel kernel's VALUES exactly:
    the sum runs in that kernel's order (bias, ci, dy, dx; every multiply-add fused in both, same flags), and each of the 45
    further terms is fma(v, 0, acc) = acc for finite v.  (Values, not bits: -0 + 0 is +0.)"""
    g = torch.Generator().manual_seed(H * 100 + Cout)
    Bs, B = 2, 4
    x = torch.randn(Bs, 4, H, W, generator=g)
    cond = torch.cat([(torch.rand(Bs, 1, H, W, generator=g) > 0.5).float(), torch.randn(Bs, 4, H, W, generator=g)], 1)
    w = torch.randn(Cout, 9, 3, 3, generator=g) / 9
    b = torch.randn(Cout, generator=g)
    xd, cd, bd = guarded_input(x), guarded_input(cond), guarded_input(b)
    wt = guarded_input(w.reshape(Cout, 81).t().contiguous())
    out = guarded((B, H, W, Cout), torch.bfloat16)
    _lib.check(sdlib.sd_op_conv_in_cond(stream(), xd.data_ptr(), Bs, cd.data_ptr(), Bs, wt.data_ptr(), bd.data_ptr(),
                                        out.data_ptr(), B, H, W, Cout))
    torch.cuda.synchronize()
    check_guards()
    full = torch.cat([x, cond], 1)
    r64, m64 = conv3x3_nhwc_ref(torch.cat([full, full]), w, b)
    print(f"conv_in_cond {H}x{W} -> {Cout}: rel-L2 {rel_l2(out, r64):.3e}")
    assert_elementwise(out, r64, linear_bound(r64, m64, 2 * 81 + 1), f"conv_in_cond {H}x{W} Cout={Cout}", NHWC)
    # zero condition weights: the 4-channel kernel on the same latents
    w0 = w.clone()
    w0[:, 4:] = 0.0
    wt0 = guarded_input(w0.reshape(Cout, 81).t().contiguous())
    wt4 = guarded_input(w[:, :4].reshape(Cout, 36).t().contiguous())
    out0, out4 = guarded((B, H, W, Cout), torch.bfloat16), guarded((B, H, W, Cout), torch.bfloat16)
    _lib.check(sdlib.sd_op_conv_in_cond(stream(), xd.data_ptr(), Bs, cd.data_ptr(), Bs, wt0.data_ptr(), bd.data_ptr(),
                                        out0.data_ptr(), B, H, W, Cout))
    _lib.check(sdlib.sd_op_conv_in(stream(), xd.data_ptr(), Bs, wt4.data_ptr(), bd.data_ptr(), out4.data_ptr(), B, H, W, 4, Cout))
    torch.cuda.synchronize()
    check_guards()
    assert torch.isfinite(out4.float()).all() and torch.equal(out0.float(), out4.float())
    assert not torch.equal(out0.float(), out.float())


# ---------------------------------------------------------------- whole inpainting loops
@pytest.fixture(scope="module")
def env():
    from oracle.vae import VaeConfig as OC
    from sonicdiffusionbayeslab_amd.models import StableDiffusionModel
    from sonicdiffusionbayeslab_amd.vae import VaeConfig, make_synthetic_vae_state_dict
    from sonicdiffusionbayeslab_amd.weights import UNetConfig, make_synthetic_state_dict
    cfg = UNetConfig(sample_size=16)
    sd = make_synthetic_state_dict(cfg, seed=1234)
    model = StableDiffusionModel(unet_config=cfg, state_dict=dict(sd)).to("cuda:0")
    vcfg = VaeConfig(sample_size=16)
    return cfg, sd, model, OC(**dataclasses.asdict(vcfg)), make_synthetic_vae_state_dict(vcfg)


@pytest.fixture(scope="module")
def env9(env):
    """The 4-channel synthetic UNet with a 9-channel conv_in (the only parameter whose shape depends on in_channels)."""
    from sonicdiffusionbayeslab_amd.models import StableDiffusionModel
    cfg, sd, _, ovcfg, vsd = env
    cfg9 = dataclasses.replace(cfg, in_channels=9)
    sd9 = dict(sd)
    g = torch.Generator().manual_seed(99)
    sd9["conv_in.weight"] = (torch.randn(cfg.block_out_channels[0], 9, 3, 3, generator=g) / 9.0).to(torch.bfloat16).float()
    model = StableDiffusionModel(unet_config=cfg9, state_dict=dict(sd9)).to("cuda:0")
    return cfg9, sd9, model, ovcfg, vsd


def _sched(model, name, **kw):
    from sonicdiffusionbayeslab_amd.registry import schedulers_registry
    from sonicdiffusionbayeslab_amd.schedulers import PNDMConfigStub
    model.scheduler = schedulers_registry[name].from_config(PNDMConfigStub().config, **kw)
    return model.scheduler


def _image(b, h, w, seed):
    g = torch.Generator().manual_seed(seed)
    low = F.interpolate(torch.rand(b, 3, h // 16, w // 16, generator=g), size=(h, w), mode="bilinear", align_corners=False)
    return (0.8 * low + 0.2 * torch.rand(b, 3, h, w, generator=g)).clamp(0, 1)


def _mask(b, seed, size=128):
    """A box (40..101 x 30..93: its sides are no multiples of 8) joined with an irregular pattern of its own per sample (a
    thresholded smooth field and a 5-pixel stripe whose position depends on the sample); soft values on both sides of 0.5."""
    g = torch.Generator().manual_seed(seed)
    field = F.interpolate(torch.rand(b, 1, 9, 9, generator=g), size=(size, size), mode="bilinear", align_corners=False)
    m = 0.45 * torch.rand(b, 1, size, size, generator=g)                  # keep: below 0.5
    hi = 0.5 + 0.5 * torch.rand(b, 1, size, size, generator=g)            # repaint: at or above 0.5
    rep = field > 0.6
    rep[:, :, 40:101, 30:93] = True
    for i in range(b):
        rep[i, :, :, 11 + 23 * i:16 + 23 * i] = True
    return torch.where(rep, hi, m)


def _compare(e, sched_name, oracle_sched, kw, b, n, strength, gs, seed, lcm=False, deepcache=None, rescale=0.0, latents=None):
    from tests.inpaint_oracle import inpaint_loop
    cfg, sd, model, ovcfg, vsd = e
    _, pe, ne = synth_inputs(dataclasses.replace(cfg, in_channels=4), b, seed=seed)
    img, mask = _image(b, 128, 128, seed=seed + 1), _mask(b, seed + 4)
    _sched(model, sched_name, **kw)
    t_start, steps = model.img2img_steps(n, strength)
    noise = None
    if lcm:
        noise = torch.randn(max(steps - 1, 1), b, 4, 16, 16, generator=torch.Generator().manual_seed(seed + 2))
    call = dict(prompt_embeds=pe, image=img, mask_image=mask, strength=strength, num_inference_steps=n, guidance_scale=gs,
                generator=torch.Generator().manual_seed(seed + 3), output_type="latent")
    if gs > 1.0:
        call["negative_prompt_embeds"] = ne
    if lcm:
        call["step_noise"] = noise.cuda()
    if rescale:
        call["guidance_rescale"] = rescale
    if latents is not None:
        call["latents"] = latents
    helper = None
    if deepcache is not None:
        from sonicdiffusionbayeslab_amd.deepcache import DeepCacheSDHelper
        helper = DeepCacheSDHelper(pipe=model)
        helper.set_params(cache_interval=deepcache.cache_interval, cache_branch_id=deepcache.cache_branch_id)
        helper.enable()
    try:
        out, secs, x0s = model(**call)
    finally:
        if helper is not None:
            helper.disable()
    ref, ref_start, ref_steps, ref_init, ref_lmask = inpaint_loop(
        sd, oracle_cfg(cfg), vsd, ovcfg, oracle_sched, pe, ne if gs > 1.0 else None, img, mask, n, strength, gs,
        torch.Generator().manual_seed(seed + 3), lcm_noise=noise, deepcache=deepcache, latents=latents, guidance_rescale=rescale)
    assert ref_steps == steps == model.num_timesteps == len(x0s), (ref_steps, steps, model.num_timesteps, len(x0s))
    assert torch.equal(model.inpaint_latent_mask.cpu(), ref_lmask) and 0.0 < float(ref_lmask.mean()) < 1.0
    es, cs_ = rel_l2(model.img2img_start_latents, ref_start), cosine(model.img2img_start_latents, ref_start)
    er, cr = rel_l2(out.images, ref), cosine(out.images, ref)
    line = f"inpaint {cfg.in_channels}ch {sched_name} N={n} strength={strength} ({steps} steps): start rel-L2 {es:.3e} cos {cs_:.6f}"
    if ref_init is not None:
        ei, ci = rel_l2(model.inpaint_image_latents, ref_init), cosine(model.inpaint_image_latents, ref_init)
        line += f"; image latents rel-L2 {ei:.3e} cos {ci:.6f}"
    print(line + f"; final rel-L2 {er:.3e} cos {cr:.5f}")
    assert es < ENC_TOL and cs_ > ENC_COS            # nothing has compounded yet: the encoder's gate
    if ref_init is not None:
        assert ei < ENC_TOL and ci > ENC_COS
    assert er < FREE_TOL and cr > FREE_COS
    return out.images


@pytest.mark.parametrize("strength", [1.0, 0.6])
def test_inpaint_ddim_loop(env, strength):
    from oracle.schedulers import DDIMOracle
    _compare(env, "ddim_scheduler", DDIMOracle(), {}, 2, 10, strength, 7.5, seed=71)


def test_inpaint_dpm_solver_pp_loop(env):
    from oracle.schedulers import DPMSolverOracle
    kw = dict(solver_order=2, algorithm_type="dpmsolver++", final_sigmas_type="zero")
    _compare(env, "dpm_solver_scheduler", DPMSolverOracle(**kw), kw, 2, 10, 0.5, 7.5, seed=73)


def test_inpaint_lcm_loop_with_step_noise(env):
    from oracle.schedulers import LCMOracle
    _compare(env, "lcm_scheduler", LCMOracle(), {}, 2, 4, 1.0, 0.0, seed=75, lcm=True)


def test_inpaint_with_deepcache(env):
    from oracle.schedulers import DDIMOracle
    from oracle.unet import DeepCacheState
    dc = DeepCacheState(cache_interval=3, cache_branch_id=0, enabled=True)
    _compare(env, "ddim_scheduler", DDIMOracle(), {}, 2, 10, 1.0, 7.5, seed=77, deepcache=dc)
    assert env[2]._deepcache is None


def test_inpaint_with_guidance_rescale(env):
    from oracle.schedulers import DDIMOracle
    _compare(env, "ddim_scheduler", DDIMOracle(), {}, 2, 10, 1.0, 7.5, seed=79, rescale=0.7)
    assert env[2].scheduler.rescale_factors is not None


# ---------------------------------------------------------------- exact properties of the 4-channel blend
def test_blend_exact_properties(env):
    cfg, sd, model, _, _ = env
    lat, pe, ne = synth_inputs(cfg, 2, seed=81)
    _sched(model, "ddim_scheduler")
    img = _image(2, 128, 128, 82)
    t2i = dict(prompt_embeds=pe, negative_prompt_embeds=ne, latents=lat, num_inference_steps=4, guidance_scale=7.5,
               output_type="latent")
    before = model(**t2i)[0].images.clone()
    inp = dict(prompt_embeds=pe, negative_prompt_embeds=ne, image=img, num_inference_steps=4, guidance_scale=7.5,
               output_type="latent")
    # nothing to repaint: the image's own latents come back, bit for bit
    keep = model(**inp, mask_image=torch.zeros(2, 1, 128, 128), generator=torch.Generator().manual_seed(1))[0].images
    assert torch.equal(bits(keep), bits(model.inpaint_image_latents))
    # everything to repaint, from given noise: the text-to-image call from the same latents, bit for bit
    full = model(**inp, mask_image=torch.ones(2, 1, 128, 128), latents=lat, strength=1.0,
                 generator=torch.Generator().manual_seed(1))[0].images
    assert model.num_timesteps == 4 and torch.equal(bits(full), bits(before))
    # another mask, another result (the parent commit ignores mask_image: both calls are then the same img2img call)
    a = model(**inp, mask_image=_mask(2, 83), generator=torch.Generator().manual_seed(1))[0].images.clone()
    b = model(**inp, mask_image=_mask(2, 84), generator=torch.Generator().manual_seed(1))[0].images
    print(f"two masks: rel-L2 {rel_l2(a, b):.3e}")
    assert rel_l2(a, b) > 1e-2
    # and the kept region of `a` is the image's latents exactly, the repainted region is not
    lm = (model.inpaint_latent_mask >= 0.5).expand_as(b)
    assert torch.equal(b[~lm], model.inpaint_image_latents[~lm]) and not torch.equal(b[lm], model.inpaint_image_latents[lm])
    # text-to-image is untouched by the inpainting calls
    assert torch.equal(bits(model(**t2i)[0].images), bits(before))
    # "argmax" draws one Gaussian less: only the forward noise
    g1, g2 = torch.Generator().manual_seed(3), torch.Generator().manual_seed(3)
    model(**inp, mask_image=_mask(2, 83), generator=g1, sample_mode="argmax")
    torch.randn(2, 4, 16, 16, generator=g2)
    assert torch.equal(g1.get_state(), g2.get_state())


# ---------------------------------------------------------------- 9-channel UNet
def test_nine_channel_forward_without_a_condition_says_so(env9):
    """A handle of its own, on which nothing has set a condition: the wrapper refuses a forward, and so does the library;
    after a condition was set and cleared, both refuse again.  The mask channel ALONE (same masked-image latents) changes
    the forward."""
    from sonicdiffusionbayeslab_amd.unet import HipUNet2DConditionModel
    cfg9, sd9, _, _, _ = env9
    u = HipUNet2DConditionModel(cfg9, dict(sd9))
    _, pe, _ = synth_inputs(dataclasses.replace(cfg9, in_channels=4), 1, seed=5)
    u.set_deepcache(-1)
    u.set_context(pe.cuda())
    lat = torch.zeros(1, 4, 16, 16, device="cuda")
    with pytest.raises(_lib.SdHipError, match="set_inpaint_cond"):
        u.forward_latents(lat, 1, 10.0)
    out = torch.empty(1, 4, 16, 16, device="cuda")
    ws = u._workspace(1, 16, 16)
    rc = u._lib.sd_unet_forward_hw(u._handle, stream(), lat.data_ptr(), 1, 1, 16, 16, 10.0, out.data_ptr(), u._ws_ptr(ws),
                                   ws.numel() - 256, 0, -1)
    torch.cuda.synchronize()
    assert rc != 0 and b"no inpainting condition is set" in u._lib.sd_last_error()
    with pytest.raises(ValueError, match="latents must be"):
        u.forward_latents(torch.zeros(1, 9, 16, 16, device="cuda"), 1, 10.0)
    g = torch.Generator().manual_seed(6)
    lat = torch.randn(1, 4, 16, 16, generator=g).cuda()
    zl = torch.randn(1, 4, 16, 16, generator=g)
    m0 = (torch.rand(1, 1, 16, 16, generator=g) > 0.5).float()
    u.set_inpaint_cond(m0, zl)
    e0 = u.forward_latents(lat, 1, 500.0).clone()
    u.set_inpaint_cond(m0, zl)
    assert torch.equal(e0, u.forward_latents(lat, 1, 500.0))
    u.set_inpaint_cond(1.0 - m0, zl)
    d = rel_l2(u.forward_latents(lat, 1, 500.0), e0)
    print(f"9-channel forward, mask channel alone inverted: rel-L2 {d:.3e}")
    assert d > 1e-2
    u.clear_inpaint_cond()
    with pytest.raises(_lib.SdHipError, match="set_inpaint_cond"):
        u.forward_latents(lat, 1, 500.0)
    rc = u._lib.sd_unet_forward_hw(u._handle, stream(), lat.data_ptr(), 1, 1, 16, 16, 10.0, out.data_ptr(), u._ws_ptr(ws),
                                   ws.numel() - 256, 0, -1)
    torch.cuda.synchronize()
    assert rc != 0 and b"no inpainting condition is set" in u._lib.sd_last_error()


def test_nine_channel_ddim_loop(env9):
    from oracle.schedulers import DDIMOracle
    _compare(env9, "ddim_scheduler", DDIMOracle(), {}, 2, 10, 1.0, 7.5, seed=91)


def test_nine_channel_mask_and_masked_image_both_matter(env9):
    """From the same given noise (strength 1: the image latents are not read, the draws are the same), the result depends on
    the mask and on the image.  (A new mask changes the mask channel AND the masked image's latents; the mask channel alone is
    varied in test_nine_channel_forward_without_a_condition_says_so and per element in test_conv_in_cond_per_element.)  A
    pipeline that dropped the condition would return identical bits."""
    cfg9, _, model, _, _ = env9
    lat, pe, ne = synth_inputs(dataclasses.replace(cfg9, in_channels=4), 2, seed=93)
    _sched(model, "ddim_scheduler")
    call = lambda img, m: model(prompt_embeds=pe, negative_prompt_embeds=ne, image=img, mask_image=m, latents=lat,
                                num_inference_steps=4, guidance_scale=7.5, generator=torch.Generator().manual_seed(2),
                                output_type="latent")[0].images.clone()
    img, other = _image(2, 128, 128, 94), _image(2, 128, 128, 95)
    base = call(img, _mask(2, 96))
    assert model.inpaint_image_latents is None
    assert torch.equal(bits(base), bits(call(img, _mask(2, 96))))
    dm, di = rel_l2(call(img, _mask(2, 97)), base), rel_l2(call(other, _mask(2, 96)), base)
    print(f"9-channel UNet: another mask rel-L2 {dm:.3e}, another image rel-L2 {di:.3e}")
    assert dm > 1e-2 and di > 1e-2
    # the generator drew the masked-image posterior only
    g1, g2 = torch.Generator().manual_seed(4), torch.Generator().manual_seed(4)
    model(prompt_embeds=pe, negative_prompt_embeds=ne, image=img, mask_image=_mask(2, 96), latents=lat, num_inference_steps=2,
          generator=g1, output_type="latent")
    torch.randn(2, 4, 16, 16, generator=g2)
    assert torch.equal(g1.get_state(), g2.get_state())


def test_nine_channel_fp8_calibration_uses_a_fixed_condition(env9):
    """fp8 handles: the activation scales of a 9-channel UNet come from the fixed seeded latents and a fixed condition (mask
    of ones, zero masked-image latents), so an explicit calibration and the one a first inpainting call triggers agree
    exactly, whatever the call's image and mask; the calibration's condition does not stay behind for later forwards."""
    from sonicdiffusionbayeslab_amd.models import StableDiffusionModel
    cfg9, sd9, _, _, _ = env9
    a = StableDiffusionModel(unet_config=cfg9, state_dict=dict(sd9), weight_dtype="fp8").to("cuda:0")
    explicit = dict(a.calibrate_fp8())
    assert explicit and a.unet._inpaint_key is None and "calibrated" in a.weights_source
    with pytest.raises(_lib.SdHipError, match="set_inpaint_cond"):          # the calibration's condition is gone
        a.unet.forward_latents(torch.zeros(2, 4, 16, 16, device="cuda"), 2, 10.0)
    b = StableDiffusionModel(unet_config=cfg9, state_dict=dict(sd9), weight_dtype="fp8").to("cuda:0")
    _sched(b, "ddim_scheduler")
    _, pe, ne = synth_inputs(dataclasses.replace(cfg9, in_channels=4), 2, seed=98)
    out = b(prompt_embeds=pe, negative_prompt_embeds=ne, image=_image(2, 128, 128, 99), mask_image=_mask(2, 100),
            num_inference_steps=2, guidance_scale=7.5, generator=torch.Generator().manual_seed(5), output_type="latent")[0].images
    assert torch.isfinite(out).all() and b.num_timesteps == 2
    assert b.fp8_scales == explicit


# ---------------------------------------------------------------- harness
def test_ddim_method_from_yaml_with_inpaint_box(env, monkeypatch, capsys, tmp_path):
    from PIL import Image
    from sonicdiffusionbayeslab_amd import models as M
    from sonicdiffusionbayeslab_amd.config import load_config
    from sonicdiffusionbayeslab_amd.registry import methods_registry
    from sonicdiffusionbayeslab_amd.weights import UNetConfig
    cfg, sd, _, _, _ = env
    d = tmp_path / "img"
    d.mkdir()
    prompts = {}
    for i, (w, h) in enumerate(((200, 150), (130, 260))):
        arr = (_image(1, 256, 256, 70 + i)[0, :, :h, :w].permute(1, 2, 0) * 255).round().to(torch.uint8).numpy()
        Image.fromarray(arr).save(str(d / f"p{i}.png"))
        prompts[f"p{i}.png"] = f"a picture, number {i}"
    (tmp_path / "prompts.json").write_text(json.dumps(prompts))
    seen = []
    real = M.StableDiffusionModel._call_inpaint

    def spy(self, prompt, image, mask_image, strength, *a):
        seen.append((tuple(mask_image.shape), float(mask_image.sum()), strength))
        return real(self, prompt, image, mask_image, strength, *a)
    monkeypatch.setattr(M.StableDiffusionModel, "_call_inpaint", spy)
    monkeypatch.setattr(M.StableDiffusionModel, "from_pretrained",
                        classmethod(lambda c, *a, **k: c(unet_config=UNetConfig(sample_size=16), state_dict=dict(sd))))
    (tmp_path / "inpaint.yaml").write_text(f"""
experiment_name: DDIM inpaint
experiment: {{method: ddim, seed: 29}}
model: {{model_name: stable_diffusion_model, pretrained_model: runwayml/stable-diffusion-v1-5}}
scheduler: {{scheduler_name: ddim_scheduler}}
dataset: {{img_dataset: "{d}", prompts: "{tmp_path / 'prompts.json'}", image_size: 128}}
inference: {{batch_size: 2, output_type: latent}}
experiment_params: {{num_inference_steps: [4], inpaint_box: [16, 24, 96, 128]}}
""")
    m = methods_registry["ddim"](load_config(str(tmp_path / "inpaint.yaml")))
    m.run_experiment()
    lines = [json.loads(l) for l in capsys.readouterr().out.splitlines() if l.startswith("{")]
    assert len(lines) == 1 and lines[0]["nfe"] == 4 and lines[0]["images"] == 2 and lines[0]["time_metric_s_per_image"] > 0
    assert seen == [((2, 1, 128, 128), 2.0 * 80 * 104, 1.0)]
