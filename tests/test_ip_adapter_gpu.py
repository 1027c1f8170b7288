"""GPU parity of IP-Adapter image prompts (diffusers IPAdapterAttnProcessor2_0 + ImageProjection, one adapter, 4 tokens).

Operator level: ``sd_op_ip_xattn`` in guarded buffers, every element against float64 from the operands the kernel reads, with
an a-priori bound (below).  UNet / loops: against the CPU oracle conditioned by tests/ip_adapter_oracle.py under the
tolerances of the plain path (UNET_TOL per forward as tests/test_unet_gpu.py, FREE_TOL / FREE_COS for free-running loops as
tests/test_pipeline_gpu.py, FWD_TOL of tests/test_fp8_gpu.py for the fp8 handle).  Without an image prompt the handle runs
today's plans: bit-identical to a handle built without adapter fields.

The operator bound and its two operand families are stated in tests/ip_xattn_case.py."""
import dataclasses

import pytest
import torch

pytestmark = pytest.mark.gpu

from sonicdiffusionbayeslab_amd import _lib
from tests.bounds import assert_elementwise, check_guards, forget_guards, guarded, guarded_input
from tests.ip_adapter_oracle import cfg_image_embeds, ip_adapter_oracle
from tests.ip_xattn_case import EPS, FAMILIES, SHAPES, operands, ref_bound
from tests.util import cosine, oracle_cfg, rel_l2, synth_inputs

UNET_TOL = 2e-2                     # tests/test_unet_gpu.py
FREE_TOL, FREE_COS = 6e-2, 0.998    # tests/test_pipeline_gpu.py
FP8_FWD_TOL = 1.5e-1                # tests/test_fp8_gpu.py: FWD_TOL
E = 1024                            # image_embeds width of the published adapter
T = 4

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


# ---------------------------------------------------------------------------------------------------------------------
# operator level
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("UB,rps,C,heads", SHAPES)
def test_ip_xattn_per_element(sdlib, UB, rps, C, heads, family):
    """Every element against float64 under the a-priori bound of tests/ip_xattn_case.py, on both operand families: ``dense``
    exercises every load, ``sharp`` is where the bound is a few per cent of the image branch and the LayerNorm / softmax
    arithmetic is what is checked (tests/test_ip_adapter_cpu.py shows that wrong kernels violate it there)."""
    M = UB * rps
    r, A, Bt, gamma, beta = operands(UB, rps, C, heads, family)
    out = guarded((M, C), torch.bfloat16, label="Rout")
    _lib.check(sdlib.sd_op_ip_xattn(stream(), P(guarded_input(r, torch.bfloat16, label="R")), P(out),
                                    P(guarded_input(A.view(UB * 32, C), torch.bfloat16, label="A")),
                                    P(guarded_input(Bt.view(UB * C, 32), torch.bfloat16, label="Bt")),
                                    P(guarded_input(gamma, torch.float32, label="gamma")),
                                    P(guarded_input(beta, torch.float32, label="beta")), EPS, M, C, rps, heads, T))
    torch.cuda.synchronize()
    y, bound, branch = ref_bound(r, A, Bt, gamma, beta, EPS, UB, rps, C, heads)
    got = out.float().cpu().view(UB, rps, C)
    rms = branch.pow(2).mean().sqrt().item()
    print(f"ip_xattn {family} UB={UB} rows={rps} C={C} heads={heads}: branch rms {rms:.3f}, median bound {bound.median().item():.4f}, "
          f"worst |err| / bound {((got.double() - y).abs() / bound).max().item():.3f}")
    assert_elementwise(got, y, bound, f"ip_xattn {family} UB={UB} rows={rps} C={C} heads={heads}", ("b", "row", "c"))
    moved = (got - r.view(UB, rps, C)).abs().max().item()
    assert moved > 0.05, "the image branch must move the residual in this test"
    check_guards()


# ---------------------------------------------------------------------------------------------------------------------
# UNet level: 32x32 latents at SD-1.5 widths = 1024 / 256 / 64 / 16 tokens per sample, all three cross-attention forms
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def weights():
    from sonicdiffusionbayeslab_amd.weights import UNetConfig, make_synthetic_ip_adapter_state_dict, make_synthetic_state_dict
    cfg = UNetConfig(sample_size=32, ip_adapter_embed_dim=E)
    sd = make_synthetic_state_dict(cfg, seed=1234)
    ipsd = make_synthetic_ip_adapter_state_dict(cfg, seed=1234)
    return cfg, sd, ipsd


@pytest.fixture(scope="module")
def nets(weights):
    from sonicdiffusionbayeslab_amd.unet import HipUNet2DConditionModel
    from sonicdiffusionbayeslab_amd.weights import without_ip_adapter
    cfg, sd, ipsd = weights
    net = HipUNet2DConditionModel(cfg, {**sd, **ipsd})
    plain = HipUNet2DConditionModel(without_ip_adapter(cfg), sd)
    return net, plain


def _embeds(n, seed=3):
    return torch.randn(n, E, generator=torch.Generator().manual_seed(seed))


@pytest.mark.parametrize("t", [981.0, 21.0])
@pytest.mark.parametrize("cfg_pair", [False, True])
def test_unet_forward_with_image_prompt_matches_oracle(weights, nets, t, cfg_pair):
    from oracle.unet import unet_forward
    cfg, sd, ipsd = weights
    net, _ = nets
    w = {**sd, **ipsd}
    lat, pe, ne = synth_inputs(cfg, 2)
    emb = cfg_image_embeds(_embeds(2), cfg_pair)                      # CFG: the negative half from zero embeds
    ctx = torch.cat([ne, pe]) if cfg_pair else pe
    ub = ctx.shape[0]
    lat_in = torch.cat([lat, lat]) if cfg_pair else lat
    with torch.no_grad():
        off = unet_forward(sd, oracle_cfg(cfg), lat_in, t, ctx)
        with ip_adapter_oracle(w, emb, 1.0):
            ref = unet_forward(w, oracle_cfg(cfg), lat_in, t, ctx)
    apart = rel_l2(ref, off)
    print(f"oracle, adapter on vs off: rel-L2 {apart:.3e}")
    assert apart > 10 * UNET_TOL                                       # the oracle alone: the adapter is not a no-op here
    net.set_deepcache(-1)
    net.set_context(ctx.cuda())
    net.clear_ip_adapter()
    eps_off = net.forward_latents(lat.cuda(), ub, t).clone()
    net.set_ip_adapter(emb, 1.0)
    eps = net.forward_latents(lat.cuda(), ub, t).clone()               # (ub = 2 x latents: the CFG dedup prefix is in play)
    torch.cuda.synchronize()
    net.clear_ip_adapter()
    err, err_off = rel_l2(eps, ref), rel_l2(eps_off, off)
    print(f"forward t={t} cfg={cfg_pair}: with image prompt rel-L2 {err:.3e} cos {cosine(eps, ref):.5f}; without {err_off:.3e}")
    assert torch.isfinite(eps).all() and err < UNET_TOL and err_off < UNET_TOL
    assert rel_l2(eps, eps_off) > 10 * UNET_TOL


def test_one_forward_at_32x40_with_tails_at_every_level(weights, nets):
    from oracle.unet import unet_forward
    cfg, sd, ipsd = weights
    net, _ = nets
    w = {**sd, **ipsd}
    g = torch.Generator().manual_seed(61)
    lat = torch.randn(1, 4, 32, 40, generator=g)                      # 1280 / 320 / 80 / 20 tokens per sample
    pe = torch.randn(1, 77, 768, generator=g)
    emb = _embeds(1, seed=8)
    net.set_deepcache(-1)
    net.set_context(pe.cuda(), 32, 40)
    net.set_ip_adapter(emb, 0.8, 32, 40)
    eps = net.forward_latents(lat.cuda(), 1, 499.0).clone()
    torch.cuda.synchronize()
    net.clear_ip_adapter()
    with torch.no_grad(), ip_adapter_oracle(w, emb, 0.8):
        ref = unet_forward(w, oracle_cfg(cfg), lat, 499.0, pe)
    err = rel_l2(eps, ref)
    print(f"32x40 forward with image prompt: rel-L2 {err:.3e} cos {cosine(eps, ref):.5f}")
    assert torch.isfinite(eps).all() and err < UNET_TOL


def test_identity_and_launch_accounting(weights, nets):
    cfg, sd, ipsd = weights
    net, plain = nets
    lat, pe, ne = synth_inputs(cfg, 2, seed=5)
    ctx = torch.cat([ne, pe]).cuda()
    emb = cfg_image_embeds(_embeds(2, seed=6))
    x = lat.cuda()
    for n in (net, plain):
        n.set_deepcache(-1)
        n.set_context(ctx)
    ref = plain.forward_latents(x, 4, 501.0).clone()
    net.clear_ip_adapter()
    never = net.forward_latents(x, 4, 501.0).clone()                  # adapter weights in the handle, no image prompt set
    net.set_ip_adapter(emb, 0.0)
    zero = net.forward_latents(x, 4, 501.0).clone()
    net.set_ip_adapter(emb, 1.0)
    on = net.forward_latents(x, 4, 501.0).clone()
    prof_on = net.forward_profiled(x, 4, 501.0)
    net.clear_ip_adapter()
    cleared = net.forward_latents(x, 4, 501.0).clone()
    prof_cleared = net.forward_profiled(x, 4, 501.0)
    prof_plain = plain.forward_profiled(x, 4, 501.0)
    torch.cuda.synchronize()
    assert torch.equal(never, ref) and torch.equal(cleared, ref) and torch.equal(zero, ref)
    assert rel_l2(on, ref) > 10 * UNET_TOL
    launches = lambda p: {k: v["launches"] for k, v in p.items()}
    assert launches(prof_cleared) == launches(prof_plain) and "ip_xattn" not in launches(prof_plain)
    lo = launches(prof_on)
    assert lo.pop("ip_xattn") == 16                                   # one per executed transformer block
    assert lo == launches(prof_plain)                                 # every other kind unchanged
    # a forward while an image prompt is set for ANOTHER batch fails and says so (the handle, below the wrapper's own check)
    net.set_ip_adapter(emb, 1.0)
    lib, ws = net._lib, net._workspace(4)
    out = torch.empty(2, 4, 32, 32, device="cuda")
    rc = lib.sd_unet_forward_hw(net._handle, stream(), x.data_ptr(), 2, 2, 32, 32, 501.0, out.data_ptr(), net._ws_ptr(ws), ws.numel() - 256, 0, -1)
    assert rc != 0 and b"none is set for batch 2" in lib.sd_last_error()
    net.set_context(ctx[:2])                                          # the wrapper says the same for a batch it has not been set for
    with pytest.raises(_lib.SdHipError, match="set_ip_adapter"):
        net.forward_latents(x, 2, 501.0)
    net.clear_ip_adapter()


def test_forward_with_image_prompt_ignores_old_workspace_contents(weights, nets):
    """The context operands, the folded image operands, their pad slots and the scratch live in a workspace that comes from
    torch.empty: with every byte of it zero, 0xFF or NaN before set_context + set_ip_adapter, a full forward gives the same bits
    (tests/test_context_fold_gpu.py has the other handles).  32x32 latents at SD-1.5 widths: all three prompt-attention forms."""
    from tests.test_context_fold_gpu import assert_same_after_every_fill, unet_after_every_fill
    cfg, sd, ipsd = weights
    net, _ = nets
    lat, pe, ne = synth_inputs(cfg, 1, seed=15)
    ctx, x = torch.cat([ne, pe]).cuda(), lat.cuda()
    emb = cfg_image_embeds(_embeds(1, seed=16))
    net.set_deepcache(-1)
    net.clear_ip_adapter()
    try:
        outs = unet_after_every_fill(net, x, ctx, 501.0, image=(emb, 0.8))
        prof = net.forward_profiled(x, 2, 501.0)
    finally:
        net.clear_ip_adapter()
    launches = {k: v["launches"] for k, v in prof.items()}
    assert launches["ip_xattn"] == 16 and launches["xattn_fused"] == 5          # the five blocks of the 1024-token level
    assert launches["attention"] == 16 + 6                                       # 64 and 16 tokens: a prompt attention launch of their own
    assert_same_after_every_fill(outs, "IP-Adapter UNet at 32x32")


def test_diffusers_style_call_with_added_cond_kwargs(weights, nets):
    cfg, sd, ipsd = weights
    net, plain = nets
    lat, pe, _ = synth_inputs(cfg, 2, seed=3)
    ctx, x, emb = pe.cuda(), lat.cuda(), _embeds(2, seed=12).cuda()
    net.set_deepcache(-1)
    net.ip_adapter_scale = 0.6
    a = net(x, torch.tensor(501), encoder_hidden_states=ctx, added_cond_kwargs={"image_embeds": emb})[0].clone()
    a3 = net(x, 501, encoder_hidden_states=ctx, added_cond_kwargs={"image_embeds": [emb[:, None]]})[0].clone()
    net.set_context(ctx)
    net.set_ip_adapter(emb, 0.6)
    b = net.forward_latents(x, 2, 501.0).clone()
    none = net(x, 501, encoder_hidden_states=ctx)[0].clone()           # no added_cond_kwargs: no image prompt
    p = plain(x, 501, encoder_hidden_states=ctx)[0].clone()
    torch.cuda.synchronize()
    net.ip_adapter_scale = 1.0
    assert torch.equal(a, b) and torch.equal(a3, b) and torch.equal(none, p) and rel_l2(a, p) > 10 * UNET_TOL
    with pytest.raises(NotImplementedError):
        plain(x, 501, encoder_hidden_states=ctx, added_cond_kwargs={"image_embeds": emb})
    with pytest.raises(NotImplementedError):
        net(x, 501, encoder_hidden_states=ctx, added_cond_kwargs={})


def test_fp8_handle_forward_with_image_prompt(weights):
    """The image branch runs in bf16 on an fp8 handle, like the prompt cross-attention; static default scales."""
    from oracle.fp8 import Fp8Emulation
    from oracle.unet import unet_forward
    from sonicdiffusionbayeslab_amd.unet import HipUNet2DConditionModel
    cfg, sd, ipsd = weights
    cfg16 = dataclasses.replace(cfg, sample_size=16)
    w = {**sd, **ipsd}
    net = HipUNet2DConditionModel(cfg16, w, weight_dtype="fp8")
    lat, pe, ne = synth_inputs(cfg16, 1)
    ctx = torch.cat([ne, pe])
    emb = cfg_image_embeds(_embeds(1, seed=21))
    with torch.no_grad(), ip_adapter_oracle(w, emb, 1.0):
        ref_q = unet_forward(w, oracle_cfg(cfg16), torch.cat([lat, lat]), 981.0, ctx, fq=Fp8Emulation(sd))
    net.set_context(ctx.cuda())
    net.set_ip_adapter(emb, 1.0)
    eps = net.forward_latents(lat.cuda(), 2, 981.0)
    torch.cuda.synchronize()
    e_q = rel_l2(eps, ref_q)
    print(f"fp8 forward with image prompt: vs emulating oracle {e_q:.3e} cos {cosine(eps, ref_q):.5f}")
    assert torch.isfinite(eps).all() and e_q < FP8_FWD_TOL


# ---------------------------------------------------------------------------------------------------------------------
# pipelines (16x16 latents)
# ---------------------------------------------------------------------------------------------------------------------
def _sched(name, **kw):
    from sonicdiffusionbayeslab_amd.registry import schedulers_registry
    from sonicdiffusionbayeslab_amd.schedulers import PNDMConfigStub
    return schedulers_registry[name].from_config(PNDMConfigStub().config, **kw)


@pytest.fixture(scope="module")
def adapter_file(weights, tmp_path_factory):
    """The synthetic adapter as a checkpoint file in the upstream layout (bf16: the values are on that grid)."""
    from sonicdiffusionbayeslab_amd.weights import to_upstream_ip_adapter
    cfg, sd, ipsd = weights
    path = tmp_path_factory.mktemp("ip_adapter") / "models" / "ip-adapter_sd15.bin"
    path.parent.mkdir()
    torch.save({g: {k: v.to(torch.bfloat16) for k, v in d.items()} for g, d in to_upstream_ip_adapter(ipsd, cfg).items()}, str(path))
    return path


def _model(weights, adapter_file, key="stable_diffusion_model", **kw):
    from sonicdiffusionbayeslab_amd.registry import models_registry
    from sonicdiffusionbayeslab_amd.weights import without_ip_adapter
    cfg, sd, ipsd = weights
    m = models_registry[key](unet_config=dataclasses.replace(without_ip_adapter(cfg), sample_size=16), state_dict=dict(sd), **kw)
    m.load_ip_adapter(str(adapter_file.parent.parent), subfolder="models", weight_name=adapter_file.name)
    assert m.unet_config.ip_adapter_embed_dim == E and "IP-Adapter(local:" in m.weights_source
    return m.to("cuda:0")


@pytest.fixture(scope="module")
def pipe(weights, adapter_file):
    return _model(weights, adapter_file)


def test_text_to_image_two_ddim_steps(weights, pipe):
    from oracle.pipeline import sample_loop
    from oracle.schedulers import DDIMOracle
    cfg, sd, ipsd = weights
    cfg16, w = dataclasses.replace(cfg, sample_size=16), {**sd, **ipsd}
    pipe.scheduler = _sched("ddim_scheduler")
    lat, pe, ne = synth_inputs(cfg16, 2, seed=41)
    emb = _embeds(2, seed=42)
    pipe.set_ip_adapter_scale(0.7)
    out, _, _ = pipe(prompt_embeds=pe, negative_prompt_embeds=ne, latents=lat, num_inference_steps=2, guidance_scale=7.5,
                     output_type="latent", ip_adapter_image_embeds=[emb[:, None]])
    out2, _, _ = pipe(prompt_embeds=pe, negative_prompt_embeds=ne, latents=lat, num_inference_steps=2, guidance_scale=7.5,
                      output_type="latent", ip_adapter_image_embeds=cfg_image_embeds(emb))        # [2 B, E], negative first
    plain, _, _ = pipe(prompt_embeds=pe, negative_prompt_embeds=ne, latents=lat, num_inference_steps=2, guidance_scale=7.5,
                       output_type="latent")
    pipe.set_ip_adapter_scale(1.0)
    with ip_adapter_oracle(w, cfg_image_embeds(emb), 0.7):
        ref, _, _, _ = sample_loop(w, oracle_cfg(cfg16), DDIMOracle(), pe, ne, lat, 2, 7.5)
    ref_plain, _, _, _ = sample_loop(sd, oracle_cfg(cfg16), DDIMOracle(), pe, ne, lat, 2, 7.5)
    err, cs = rel_l2(out.images, ref), cosine(out.images, ref)
    print(f"text-to-image DDIM 2 steps with image prompt: rel-L2 {err:.3e} cos {cs:.5f}; without: {rel_l2(plain.images, ref_plain):.3e}")
    assert err < FREE_TOL and cs > FREE_COS and torch.equal(out2.images, out.images)
    assert rel_l2(plain.images, ref_plain) < FREE_TOL and not torch.equal(plain.images, out.images)


def test_deepcache_full_and_skip_step(weights, pipe):
    from oracle.pipeline import sample_loop
    from oracle.schedulers import DDIMOracle
    from oracle.unet import DeepCacheState
    from sonicdiffusionbayeslab_amd.deepcache import DeepCacheSDHelper
    cfg, sd, ipsd = weights
    cfg16, w = dataclasses.replace(cfg, sample_size=16), {**sd, **ipsd}
    pipe.scheduler = _sched("ddim_scheduler")
    lat, pe, _ = synth_inputs(cfg16, 2, seed=43)
    emb = _embeds(2, seed=44)
    helper = DeepCacheSDHelper(pipe=pipe)
    helper.set_params(cache_interval=2, cache_branch_id=0)
    helper.enable()
    try:
        out, _, _ = pipe(prompt_embeds=pe, latents=lat, num_inference_steps=2, guidance_scale=1.0, output_type="latent",
                         ip_adapter_image_embeds=emb)
        prof_skip = pipe.unet.forward_profiled(lat.cuda(), 2, 501.0, cache_mode=2)
    finally:
        helper.disable()
    dc = DeepCacheState(cache_interval=2, cache_branch_id=0, enabled=True)
    with ip_adapter_oracle(w, emb, 1.0):
        ref, _, _, _ = sample_loop(w, oracle_cfg(cfg16), DDIMOracle(), pe, None, lat, 2, 1.0, deepcache=dc)
    err, cs = rel_l2(out.images, ref), cosine(out.images, ref)
    print(f"DeepCache N=2 branch 0 (one full, one skip step) with image prompt: rel-L2 {err:.3e} cos {cs:.5f}")
    assert err < FREE_TOL and cs > FREE_COS
    assert prof_skip["ip_xattn"]["launches"] == 1                      # branch 0: only the outermost up layer's transformer block runs


def test_img2img_two_steps(weights, pipe):
    from oracle.schedulers import DDIMOracle
    from oracle.vae import VaeConfig as OC
    from sonicdiffusionbayeslab_amd.vae import VaeConfig, make_synthetic_vae_state_dict
    from tests.vae_encoder_oracle import img2img_loop
    cfg, sd, ipsd = weights
    cfg16, w = dataclasses.replace(cfg, sample_size=16), {**sd, **ipsd}
    vcfg = VaeConfig(sample_size=16)
    vsd = make_synthetic_vae_state_dict(vcfg)
    pipe.scheduler = _sched("ddim_scheduler")
    _, pe, ne = synth_inputs(cfg16, 1, seed=45)
    img = torch.rand(1, 3, 128, 128, generator=torch.Generator().manual_seed(46))
    emb = _embeds(1, seed=47)
    out, _, x0s = pipe(prompt_embeds=pe, negative_prompt_embeds=ne, image=img, strength=0.5, num_inference_steps=4, guidance_scale=7.5,
                       generator=torch.Generator().manual_seed(48), output_type="latent", ip_adapter_image_embeds=emb)
    with ip_adapter_oracle(w, cfg_image_embeds(emb), 1.0):
        ref, _, steps = img2img_loop(w, oracle_cfg(cfg16), vsd, OC(**dataclasses.asdict(vcfg)), DDIMOracle(), pe, ne, img, 4, 0.5, 7.5,
                                     torch.Generator().manual_seed(48))
    err, cs = rel_l2(out.images, ref), cosine(out.images, ref)
    print(f"img2img DDIM ({steps} steps) with image prompt: rel-L2 {err:.3e} cos {cs:.5f}")
    assert steps == 2 == len(x0s) and err < FREE_TOL and cs > FREE_COS


def test_skip_timesteps_variant(weights, adapter_file):
    from oracle.pipeline import sample_loop_skip
    from oracle.schedulers import DDIMOracle
    cfg, sd, ipsd = weights
    cfg16, w = dataclasses.replace(cfg, sample_size=16), {**sd, **ipsd}
    m = _model(weights, adapter_file, "stable_diffusion_model_skip_timesteps")
    m.scheduler = _sched("ddim_scheduler")
    lat, pe, ne = synth_inputs(cfg16, 1, seed=49)
    emb = _embeds(1, seed=50)
    out, _, _ = m(prompt_embeds=pe, negative_prompt_embeds=ne, latents=lat, guidance_scale=7.5, num_inference_steps=3, skip_timesteps=[1],
                  output_type="latent", ip_adapter_image_embeds=emb)
    with ip_adapter_oracle(w, cfg_image_embeds(emb), 1.0):
        ref, _, used = sample_loop_skip(w, oracle_cfg(cfg16), DDIMOracle(), pe, ne, lat, 3, [1], 7.5)
    err, cs = rel_l2(out.images, ref), cosine(out.images, ref)
    print(f"skip-timesteps variant ({len(used)} steps) with image prompt: rel-L2 {err:.3e} cos {cs:.5f}")
    assert err < FREE_TOL and cs > FREE_COS


def test_ip_adapter_image_equals_the_call_with_its_embeds(weights, adapter_file):
    """``ip_adapter_image`` goes through a small CLIP vision tower of the kind the HIP tower builds (head dim 64, quick_gelu):
    bit for bit the call with the embeds ``HipClipVisionModel`` returns for the same images."""
    import json
    from safetensors.torch import save_file
    from sonicdiffusionbayeslab_amd.clip_score import ClipVisionConfig, HipClipVisionModel, make_synthetic_clip_vision_state_dict
    cfg, sd, ipsd = weights
    cfg16 = dataclasses.replace(cfg, sample_size=16)
    vcfg = ClipVisionConfig(hidden_size=128, num_hidden_layers=2, num_attention_heads=2, intermediate_size=256, image_size=224,
                            patch_size=32, projection_dim=E)
    vsd = make_synthetic_clip_vision_state_dict(vcfg, seed=7)
    enc = adapter_file.parent / "image_encoder"          # where upstream resolves image_encoder_folder: beside the subfolder's file
    enc.mkdir()
    (enc / "config.json").write_text(json.dumps({**dataclasses.asdict(vcfg), "hidden_act": "quick_gelu"}))
    save_file({k: v.contiguous() for k, v in vsd.items()}, str(enc / "model.safetensors"))
    m = _model(weights, adapter_file)
    assert m._ip_encoder_dir == str(enc)
    m.scheduler = _sched("ddim_scheduler")
    lat, pe, ne = synth_inputs(cfg16, 2, seed=51)
    imgs = torch.randint(0, 256, (2, 3, 96, 80), generator=torch.Generator().manual_seed(52), dtype=torch.uint8)
    kw = dict(prompt_embeds=pe, negative_prompt_embeds=ne, latents=lat, num_inference_steps=1, guidance_scale=7.5, output_type="latent")
    a, _, _ = m(ip_adapter_image=imgs, **kw)
    emb = HipClipVisionModel(vcfg, vsd)(imgs.cuda())
    assert torch.equal(m.ip_adapter_image_embeds, torch.cat([torch.zeros_like(emb), emb]))        # the negative half is zeros
    b, _, _ = m(ip_adapter_image_embeds=emb, **kw)
    c, _, _ = m(**kw)
    assert torch.equal(a.images, b.images) and not torch.equal(a.images, c.images)


# ---------------------------------------------------------------------------------------------------------------------
# the image encoder's tower: head dim 80 and exact GELU (CLIP ViT-H/14)
# ---------------------------------------------------------------------------------------------------------------------
VIT_TOL = 1.5e-2                    # tests/test_clip_score_gpu.py: TOL of the tiny tower against transformers


def test_vision_tower_head_dim_80_exact_gelu_matches_transformers():
    """Two layers with the published encoder's head dim (80), activation (exact gelu), patch size (14) and token count (257),
    against transformers' CLIPVisionModelWithProjection on the same config and weights.  At the embedding the two activations
    are only ~1e-2 apart (the LayerNorms absorb most of it), below the gate; so the test also runs both towers with
    quick_gelu and checks that the HIP towers' difference points where transformers' does: a tower that ignored
    ``hidden_act`` would leave only rounding noise there (cosine ~ 0)."""
    from transformers import CLIPVisionConfig, CLIPVisionModelWithProjection
    from sonicdiffusionbayeslab_amd.clip_score import ClipVisionConfig, HipClipVisionModel, make_synthetic_clip_vision_state_dict
    from tests.clip_score_util import tiny_images
    from tests.clip_vision_oracle import pil_crop, pixel_values
    shape = dict(hidden_size=320, num_hidden_layers=2, num_attention_heads=4, intermediate_size=640, image_size=224, patch_size=14,
                 projection_dim=256)
    vsd = make_synthetic_clip_vision_state_dict(ClipVisionConfig(**shape), seed=9)
    # a stronger MLP branch (fc2 x 4, still on the bf16 grid), so that the activation carries weight in the embedding
    vsd = {n: ((4.0 * v).to(torch.bfloat16).float() if n.endswith("mlp.fc2.weight") else v) for n, v in vsd.items()}
    images = tiny_images()
    pix = torch.stack([pixel_values(pil_crop(im, 224)) for im in images])
    ref, got = {}, {}
    for act in ("gelu", "quick_gelu"):
        model = CLIPVisionModelWithProjection(CLIPVisionConfig(hidden_act=act, layer_norm_eps=1e-5, **shape)).eval()
        res = model.load_state_dict(vsd, strict=False)
        assert not res.unexpected_keys and all("position_ids" in k for k in res.missing_keys), res
        with torch.no_grad():
            ref[act] = model(pixel_values=pix).image_embeds
        net = HipClipVisionModel(ClipVisionConfig(hidden_act=act, **shape), vsd)
        got[act] = torch.cat([net(im[None].cuda()) for im in images]).cpu()
        if act == "gelu":
            both = net(torch.stack(images[:2]).cuda()).cpu()         # a batch of two: the sample stride of the strided q | k | v
        err = rel_l2(got[act], ref[act])
        print(f"vision tower head dim 80 + {act} vs transformers: image embeds rel-L2 {err:.3e}")
        assert torch.isfinite(got[act]).all() and err <= VIT_TOL
    apart = rel_l2(ref["quick_gelu"], ref["gelu"])
    cs = cosine(got["gelu"] - got["quick_gelu"], ref["gelu"] - ref["quick_gelu"])
    print(f"transformers gelu vs quick_gelu: rel-L2 {apart:.3e}; cosine of the HIP towers' difference with it {cs:.4f}")
    assert apart > 5e-3 and cs > 0.5
    assert rel_l2(got["gelu"], ref["gelu"]) < rel_l2(got["gelu"], ref["quick_gelu"])
    assert torch.equal(both, got["gelu"][:2])


def test_head_dim_64_quick_gelu_tower_keeps_its_bits():
    """The tower that existed before head dim 80 and exact GELU: the tiny head-dim-64 / quick_gelu tower of
    tests/clip_score_util.py on its seeded images gives, bit for bit, the embeddings recorded on the commit before the
    extension (tests/golden/vit_hd64_quick_gelu.safetensors, written by tests/golden/make_vit_hd64_golden.py)."""
    import os
    from safetensors import safe_open
    from tests.golden.make_vit_hd64_golden import NAME, embed, inputs
    vcfg, vsd, images, digest = inputs()
    with safe_open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", NAME), "pt") as f:
        assert f.metadata()["inputs_sha256"] == digest, "the seeded weights / images are not the recorded ones: the golden does not apply"
        gold_single, gold_pair = f.get_tensor("image_embeds"), f.get_tensor("pair_embeds")
    single, pair = embed(vcfg, vsd, images)
    print(f"head-dim-64 quick_gelu tower vs the recorded bits: max |d| {(single - gold_single).abs().max().item():.3e} (single), "
          f"{(pair - gold_pair).abs().max().item():.3e} (batch of two)")
    assert torch.equal(single, gold_single) and torch.equal(pair, gold_pair)

