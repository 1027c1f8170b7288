"""GPU parity of image-to-image: the AutoencoderKL encoder against the fp32 oracle (tests/vae_encoder_oracle.py) at the
decoder's gates, the asymmetric stride-2 conv and the posterior kernel per element against fp64 with a-priori bounds,
``add_noise`` against the closed form, and whole img2img loops against the restated loop at the free-running gates of
tests/test_pipeline_gpu.py."""
import dataclasses
import json
import math
import os

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from sonicdiffusionbayeslab_amd import _lib
from tests.bounds import (ATOL_TINY, U32, assert_elementwise, check_guards, forget_guards, guarded, guarded_input,
                          linear_bound)
from tests.util import cosine, oracle_cfg, rel_l2, synth_inputs

ENC_TOL, ENC_COS = 2e-2, 0.999            # the decoder's gates (tests/test_vae_gpu.py): same kernels, comparable depth
ROW_TOL = 5e-3                            # one image alone vs its row of a batch (the decoder's figure)
FREE_TOL, FREE_COS = 6e-2, 0.998          # tests/test_pipeline_gpu.py
NHWC = ("b", "y", "x", "c")


def stream():
    return torch.cuda.current_stream().cuda_stream


@pytest.fixture(autouse=True)
def _drop_guards():
    yield
    torch.cuda.synchronize()
    forget_guards()


def r16(t):
    return t.to(torch.bfloat16).float()


# ---------------------------------------------------------------- asymmetric stride-2 conv as an op
def _pack(w, Cout, Cin):
    return w.permute(0, 2, 3, 1).reshape(Cout, 9, Cin // 64, 64).permute(0, 2, 1, 3).contiguous()


# the encoder's three downsamplers (the 128-channel 512x512 one as a 128x128 crop: its fp64 reference is what is heavy),
# and an odd non-square shape with an M tail and a Cout tail
@pytest.mark.parametrize("B,H,W,Cin,Cout", [(1, 128, 128, 128, 128), (1, 256, 256, 256, 256), (1, 128, 128, 512, 512),
                                            (3, 10, 22, 64, 192)])
def test_asymmetric_stride2_conv_per_element(sdlib, B, H, W, Cin, Cout):
    g = torch.Generator().manual_seed(B * 1000 + H + Cin)
    x = r16(torch.randn(B, Cin, H, W, generator=g))
    w = r16(torch.randn(Cout, Cin, 3, 3, generator=g) / math.sqrt(9 * Cin))
    b = torch.randn(Cout, generator=g)
    xd = guarded_input(x.permute(0, 2, 3, 1).contiguous(), torch.bfloat16)
    wd = guarded_input(_pack(w, Cout, Cin), torch.bfloat16)
    bd = guarded_input(b)
    # the UNet's symmetric stride-2 conv on the same operands, before and after the asymmetric call: bit-identical
    sym0 = guarded((B, H // 2, W // 2, Cout), torch.bfloat16)
    _lib.check(sdlib.sd_op_conv3x3(stream(), xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), None, None, sym0.data_ptr(), B, H, W,
                                   Cin, Cout, 2, 0))
    out = guarded((B, H // 2, W // 2, Cout), torch.bfloat16)
    _lib.check(sdlib.sd_op_conv3x3_down_asym(stream(), xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), out.data_ptr(), B, H, W,
                                             Cin, Cout))
    sym1 = guarded((B, H // 2, W // 2, Cout), torch.bfloat16)
    _lib.check(sdlib.sd_op_conv3x3(stream(), xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), None, None, sym1.data_ptr(), B, H, W,
                                   Cin, Cout, 2, 0))
    torch.cuda.synchronize()
    check_guards()
    assert torch.equal(sym0.view(torch.int16), sym1.view(torch.int16))
    xp, wp = F.pad(x.double(), (0, 1, 0, 1)), w.double()
    r64 = (F.conv2d(xp, wp, None, stride=2) + b.double()[None, :, None, None]).permute(0, 2, 3, 1)
    m64 = (F.conv2d(xp.abs(), wp.abs(), None, stride=2) + b.double().abs()[None, :, None, None]).permute(0, 2, 3, 1)
    assert r64.shape == (B, H // 2, W // 2, Cout)
    print(f"asym conv B={B} {H}x{W} {Cin}->{Cout}: rel-L2 {rel_l2(out, r64):.3e}")
    assert_elementwise(out, r64, linear_bound(r64, m64, 9 * Cin + 3), f"asym stride-2 conv B={B} {H}x{W} {Cin}->{Cout}", NHWC)
    # the symmetric one still is F.conv2d(..., stride=2, padding=1)
    s64 = (F.conv2d(x.double(), wp, None, stride=2, padding=1) + b.double()[None, :, None, None]).permute(0, 2, 3, 1)
    sm64 = (F.conv2d(x.double().abs(), wp.abs(), None, stride=2, padding=1) + b.double().abs()[None, :, None, None]).permute(0, 2, 3, 1)
    assert_elementwise(sym1, s64, linear_bound(s64, sm64, 9 * Cin + 3), f"symmetric stride-2 conv B={B} {H}x{W} {Cin}->{Cout}", NHWC)


# ---------------------------------------------------------------- posterior kernel
def test_posterior_kernel_per_element(sdlib):
    """z = s (m + exp(0.5 clamp(l, -30, 20)) n) in fp32.  A-priori bound, U = 2^-24 the fp32 unit roundoff:
    0.5 * l is exact; expf returns exp(h) (1 + d1) with |d1| <= 1 ulp <= 2 U (HIP math API: expf, maximum error 1 ulp);
    the product e n rounds once (U), the sum m + e n rounds once (U) -- or both round once as an fma, which is no worse --
    and the scale multiplies and rounds once (U).  To first order
        |z_hat - z| <= |s| (3 U |e n| + 2 U |m + e n|),
    taken with 1 % of slack for the second-order terms."""
    g = torch.Generator().manual_seed(11)
    B, hw = 3, 16 * 24
    mean = torch.randn(B, 4, hw, generator=g) * 3.0
    logvar = torch.randn(B, 4, hw, generator=g) * 6.0 - 4.0
    logvar[0, 0, :8] = torch.tensor([-40.0, 25.0, -30.0, 20.0, -30.000002, 20.000002, 0.0, -100.0])     # both clamps, and their edges
    noise = torch.randn(B, 4, hw, generator=g)
    scale = 0.18215
    s32 = float(torch.tensor(scale, dtype=torch.float32))            # what the kernel receives
    mom = guarded_input(torch.cat([mean, logvar], 1).contiguous())
    nz = guarded_input(noise)
    out = guarded((B, 4, hw), torch.float32)
    _lib.check(sdlib.sd_vae_posterior_sample(stream(), mom.data_ptr(), nz.data_ptr(), scale, out.data_ptr(), B, hw))
    mode = guarded((B, 4, hw), torch.float32)
    _lib.check(sdlib.sd_vae_posterior_sample(stream(), mom.data_ptr(), None, scale, mode.data_ptr(), B, hw))
    torch.cuda.synchronize()
    check_guards()
    m, l, n = mean.double(), logvar.double().clamp(-30.0, 20.0), noise.double()
    en = torch.exp(0.5 * l) * n
    ref = s32 * (m + en)
    bound = 1.01 * abs(s32) * (3 * U32 * en.abs() + 2 * U32 * (m + en).abs()) + ATOL_TINY
    assert_elementwise(out, ref, bound, "posterior sample", ("b", "c", "p"))
    assert_elementwise(mode, s32 * m, 1.01 * U32 * (s32 * m).abs() + ATOL_TINY, "posterior mode", ("b", "c", "p"))


# ---------------------------------------------------------------- encoder against the fp32 oracle
@pytest.fixture(scope="module")
def vae():
    from oracle.vae import VaeConfig as OC
    from sonicdiffusionbayeslab_amd.vae import HipVaeEncoder, VaeConfig, make_synthetic_vae_state_dict
    cfg = VaeConfig(sample_size=16)
    sd = make_synthetic_vae_state_dict(cfg)
    return cfg, OC(**dataclasses.asdict(cfg)), sd, HipVaeEncoder(cfg, sd)


def _image(b, h, w, seed):
    """A smooth picture plus texture in [0, 1] (a uniform-noise image has no structure for the downsamplers to keep)."""
    g = torch.Generator().manual_seed(seed)
    low = F.interpolate(torch.rand(b, 3, h // 16, w // 16, generator=g), size=(h, w), mode="bilinear", align_corners=False)
    return (0.8 * low + 0.2 * torch.rand(b, 3, h, w, generator=g)).clamp(0, 1)


def _gate(got, ref, what):
    out = []
    for name, sl in (("mean", slice(0, 4)), ("logvar", slice(4, 8))):
        e, c = rel_l2(got[:, sl], ref[:, sl]), cosine(got[:, sl], ref[:, sl])
        print(f"VAE encode {what} {name}: rel-L2 {e:.3e} cos {c:.6f}")
        out.append((name, e, c))
    for name, e, c in out:
        assert e < ENC_TOL and c > ENC_COS, (what, name, e, c)


@pytest.mark.parametrize("b,h,w", [(2, 128, 128), (2, 128, 192), (1, 512, 512)])
def test_vae_encoder_matches_oracle(vae, b, h, w):
    from tests.vae_encoder_oracle import vae_encode
    cfg, ocfg, sd, enc = vae
    img = _image(b, h, w, seed=h + w)
    ref = vae_encode(sd, ocfg, img)
    got = enc.encode(img.cuda())
    torch.cuda.synchronize()
    assert got.shape == (b, 8, h // 8, w // 8) and got.dtype == torch.float32 and torch.isfinite(got).all()
    _gate(got, ref, f"{b}x{h}x{w}")
    if b > 1:       # image 1 alone agrees with row 1 of the batch (split factors / GroupNorm partitions depend on the batch)
        one = enc.encode(img[1:2].cuda())
        e = rel_l2(one, got[1:2])
        print(f"VAE encode {h}x{w}: image 1 alone vs row 1 of the batch rel-L2 {e:.3e}")
        assert e < ROW_TOL


def test_encoder_sample_and_mode(vae):
    from tests.vae_encoder_oracle import posterior_sample
    cfg, ocfg, sd, enc = vae
    g = torch.Generator().manual_seed(4)
    mom = torch.randn(2, 8, 16, 24, generator=g)
    nz = torch.randn(2, 4, 16, 24, generator=g)
    assert rel_l2(enc.sample(mom.cuda(), nz), posterior_sample(mom, nz, "sample", cfg.scaling_factor)) < 1e-6
    assert rel_l2(enc.sample(mom.cuda(), mode="argmax", scale=1.0), mom[:, :4]) < 1e-7
    with pytest.raises(ValueError):
        enc.sample(mom.cuda(), mode="mean")
    with pytest.raises(ValueError):
        enc.encode(torch.rand(1, 3, 100, 128))


# ---------------------------------------------------------------- add_noise
@pytest.mark.parametrize("kind,kw,n,index", [("ddim", {}, 10, 4), ("lcm", {}, 4, 2),
                                             ("dpm", dict(solver_order=2, algorithm_type="dpmsolver++", final_sigmas_type="zero"), 10, 5)])
def test_add_noise_matches_the_closed_form(kind, kw, n, index):
    from oracle.schedulers import DDIMOracle, DPMSolverOracle, LCMOracle
    from sonicdiffusionbayeslab_amd.registry import schedulers_registry
    from sonicdiffusionbayeslab_amd.schedulers import PNDMConfigStub
    from tests.vae_encoder_oracle import add_noise_coefs
    name = {"ddim": "ddim_scheduler", "dpm": "dpm_solver_scheduler", "lcm": "lcm_scheduler"}[kind]
    s = schedulers_registry[name].from_config(PNDMConfigStub().config, **kw)
    o = {"ddim": DDIMOracle, "dpm": DPMSolverOracle, "lcm": LCMOracle}[kind](**kw)
    s.set_timesteps(n, device="cuda"); o.set_timesteps(n)
    g = torch.Generator().manual_seed(6)
    x, z = torch.randn(2, 4, 16, 24, generator=g), torch.randn(2, 4, 16, 24, generator=g)
    t = int(o.timesteps[index])
    alpha, sigma = add_noise_coefs(o, index)
    if kind != "dpm":
        ac = float(o.alphas_cumprod[t].double())
        assert alpha == math.sqrt(ac) and sigma == math.sqrt(1.0 - ac)
    got = s.add_noise(x.cuda(), z.cuda(), t)
    ref = alpha * x.double() + sigma * z.double()
    e = rel_l2(got, ref)
    print(f"add_noise {kind} t={t}: rel-L2 {e:.3e}")
    assert e < 1e-5
    assert s._step_index is None          # the multistep state is untouched


# ---------------------------------------------------------------- whole img2img loops
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


def _sched(model, name, **kw):
    from sonicdiffusionbayeslab_amd.registry import schedulers_registry
    from sonicdiffusionbayeslab_amd.schedulers import PNDMConfigStub
    model.scheduler = schedulers_registry[name].from_config(PNDMConfigStub().config, **kw)
    return model.scheduler


def _compare(env, sched_name, oracle_sched, kw, b, n, strength, gs, seed, lcm=False, deepcache=None):
    from tests.vae_encoder_oracle import img2img_loop
    cfg, sd, model, ovcfg, vsd = env
    _, pe, ne = synth_inputs(cfg, b, seed=seed)
    img = _image(b, 128, 128, seed=seed + 1)
    _sched(model, sched_name, **kw)
    t_start, steps = model.img2img_steps(n, strength)
    noise = None
    if lcm:
        noise = torch.randn(max(steps - 1, 1), b, 4, 16, 16, generator=torch.Generator().manual_seed(seed + 2))
    call = dict(prompt_embeds=pe, image=img, strength=strength, num_inference_steps=n, guidance_scale=gs,
                generator=torch.Generator().manual_seed(seed + 3), output_type="latent")
    if gs > 1.0:
        call["negative_prompt_embeds"] = ne
    if lcm:
        call["step_noise"] = noise.cuda()
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
    ref, ref_start, ref_steps = img2img_loop(sd, oracle_cfg(cfg), vsd, ovcfg, oracle_sched, pe, ne if gs > 1.0 else None, img, n,
                                             strength, gs, torch.Generator().manual_seed(seed + 3), lcm_noise=noise,
                                             deepcache=deepcache)
    assert ref_steps == steps == model.num_timesteps == len(x0s), (ref_steps, steps, model.num_timesteps, len(x0s))
    es, cs_ = rel_l2(model.img2img_start_latents, ref_start), cosine(model.img2img_start_latents, ref_start)
    e, c = rel_l2(out.images, ref), cosine(out.images, ref)
    print(f"img2img {sched_name} N={n} strength={strength} ({steps} steps): start rel-L2 {es:.3e} cos {cs_:.6f}; "
          f"final rel-L2 {e:.3e} cos {c:.5f}")
    assert es < ENC_TOL and cs_ > ENC_COS            # nothing has compounded yet: the encoder's gate
    assert e < FREE_TOL and c > FREE_COS
    return out.images


def test_img2img_ddim_loop(env):
    from oracle.schedulers import DDIMOracle
    _compare(env, "ddim_scheduler", DDIMOracle(), {}, 2, 10, 0.6, 7.5, seed=51)


def test_img2img_dpm_solver_pp_loop(env):
    from oracle.schedulers import DPMSolverOracle
    kw = dict(solver_order=2, algorithm_type="dpmsolver++", final_sigmas_type="zero")
    _compare(env, "dpm_solver_scheduler", DPMSolverOracle(**kw), kw, 1, 10, 0.5, 7.5, seed=53)


def test_img2img_lcm_loop_with_step_noise(env):
    from oracle.schedulers import LCMOracle
    _compare(env, "lcm_scheduler", LCMOracle(), {}, 2, 4, 0.5, 0.0, seed=55, lcm=True)


def test_img2img_strength_one_runs_every_step(env):
    from oracle.schedulers import DDIMOracle
    _compare(env, "ddim_scheduler", DDIMOracle(), {}, 1, 4, 1.0, 7.5, seed=57)
    assert env[2].num_timesteps == 4


def test_img2img_with_deepcache(env):
    from oracle.schedulers import DDIMOracle
    from oracle.unet import DeepCacheState
    dc = DeepCacheState(cache_interval=3, cache_branch_id=0, enabled=True)
    _compare(env, "ddim_scheduler", DDIMOracle(), {}, 1, 10, 0.7, 7.5, seed=59, deepcache=dc)
    assert env[2]._deepcache is None


def test_text_to_image_is_untouched_by_an_img2img_call(env):
    cfg, sd, model, _, _ = env
    lat, pe, ne = synth_inputs(cfg, 2, seed=61)
    _sched(model, "ddim_scheduler")
    call = dict(prompt_embeds=pe, negative_prompt_embeds=ne, latents=lat, num_inference_steps=4, guidance_scale=7.5,
                output_type="latent")
    a = model(**call)[0].images.clone()
    i2i = model(prompt_embeds=pe, negative_prompt_embeds=ne, image=_image(2, 128, 128, 62), strength=0.5,
                num_inference_steps=4, guidance_scale=7.5, generator=torch.Generator().manual_seed(1), output_type="latent")[0].images
    b = model(**call)[0].images
    assert model.num_timesteps == 4
    assert torch.equal(a, b)
    assert not torch.equal(a, i2i)
    # and the image matters: another picture, another result; "argmax" draws one Gaussian less
    other = model(prompt_embeds=pe, negative_prompt_embeds=ne, image=_image(2, 128, 128, 63), strength=0.5,
                  num_inference_steps=4, guidance_scale=7.5, generator=torch.Generator().manual_seed(1), output_type="latent")[0].images
    assert rel_l2(other, i2i) > 1e-2
    g1, g2 = torch.Generator().manual_seed(1), torch.Generator().manual_seed(1)
    model(prompt_embeds=pe, negative_prompt_embeds=ne, image=_image(2, 128, 128, 62), strength=0.5, num_inference_steps=4,
          generator=g1, output_type="latent", sample_mode="argmax")
    torch.randn(2, 4, 16, 16, generator=g2)
    assert torch.equal(g1.get_state(), g2.get_state())


# ---------------------------------------------------------------- harness
def test_ddim_method_from_yaml_with_strength(env, monkeypatch, capsys, tmp_path):
    from PIL import Image
    from sonicdiffusionbayeslab_amd import models as M
    from sonicdiffusionbayeslab_amd.config import _wrap
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
    monkeypatch.setattr(M.StableDiffusionModel, "from_pretrained",
                        classmethod(lambda c, *a, **k: c(unet_config=UNetConfig(sample_size=16), state_dict=dict(sd))))
    conf = _wrap({"experiment_name": "DDIM img2img", "experiment": {"method": "ddim", "seed": 29},
                  "model": {"model_name": "stable_diffusion_model", "pretrained_model": "runwayml/stable-diffusion-v1-5"},
                  "scheduler": {"scheduler_name": "ddim_scheduler"},
                  "dataset": {"img_dataset": str(d), "prompts": str(tmp_path / "prompts.json"), "image_size": 128},
                  "inference": {"batch_size": 2, "output_type": "latent"},
                  "experiment_params": {"num_inference_steps": [4, 10], "strength": 0.5}})
    m = methods_registry["ddim"](conf)
    m.run_experiment()
    lines = [json.loads(l) for l in capsys.readouterr().out.splitlines() if l.startswith("{")]
    assert len(lines) == 2
    assert [r["nfe"] for r in lines] == [2, 5]                 # steps actually run
    for rec in lines:
        assert rec["images"] == 2 and rec["time_metric_s_per_image"] > 0
