"""GPU parity of ControlNet (diffusers ControlNetModel, guess_mode False): the residual-add and conv_in-with-addend kernels
per element in guarded buffers against float64, the conditioning embedding, the ControlNet forward, the UNet that consumes
its residuals and the pipeline surface, against tests/controlnet_oracle.py under the tolerances of the plain path
(UNET_TOL per forward as tests/test_unet_gpu.py, FREE_TOL / FREE_COS for free-running loops as tests/test_pipeline_gpu.py).
With the residuals cleared a handle runs today's plans: bit-identical to a handle that never saw a ControlNet."""
import dataclasses
import functools
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

from sonicdiffusionbayeslab_amd import _lib
from tests.bounds import (ATOL_TINY, NHWC, assert_elementwise, check_guards, conv3x3_nhwc_ref, forget_guards, guarded,
                          guarded_input, linear_bound)
from tests.controlnet_oracle import cond_embedding, control_loop, controlnet_forward, controlnet_oracle, unet_forward_with_residuals
from tests.util import cosine, oracle_cfg, rel_l2, synth_inputs

UNET_TOL = 2e-2                     # tests/test_unet_gpu.py
FREE_TOL, FREE_COS = 6e-2, 0.998    # tests/test_pipeline_gpu.py
ENC_TOL = 2e-2                      # tests/test_img2img_gpu.py: the VAE encoder's conv stack

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


def r16(t):
    return t.to(torch.bfloat16).float()


# ---------------------------------------------------------------------------------------------------------------------
# operator level
# ---------------------------------------------------------------------------------------------------------------------
def _residual_add_case(sdlib, counts, gaps, scale, seed):
    """Segments of ``counts`` elements inside ONE guarded destination with ``gaps`` untouched elements before each; the source
    segments are packed with gaps of their own.  Every element against float64 under
    2^-8 |y| + 2^-20 (|x| + |s r|): one bf16 rounding of an fp32 evaluation."""
    g = torch.Generator().manual_seed(seed)
    dst_off, src_off, d, s = [], [], 0, 8
    for n, gap in zip(counts, gaps):
        d += gap
        dst_off.append(d); src_off.append(s)
        d = (d + n + 7) // 8 * 8                  # (segment starts are multiples of 8 elements: 16-byte vectors)
        s += (n + 15) // 8 * 8
    x = r16(torch.randn(d + 64, generator=g) * 2.0)
    r = r16(torch.randn(s + 8, generator=g))
    xd = guarded_input(x, torch.bfloat16, label="x")
    rd = guarded_input(r, torch.bfloat16, label="r")
    LL = _lib.C.c_longlong * len(counts)
    _lib.check(sdlib.sd_op_residual_add(stream(), P(xd), LL(*dst_off), P(rd), LL(*src_off), LL(*counts), len(counts), scale))
    torch.cuda.synchronize()
    got = xd.float().cpu()
    s32 = float(torch.tensor(scale, dtype=torch.float32))
    touched = torch.zeros(x.numel(), dtype=torch.bool)
    for k, (n, do, so) in enumerate(zip(counts, dst_off, src_off)):
        xs, rs = x[do:do + n].double(), r[so:so + n].double()
        y = xs + s32 * rs
        bound = 2.0 ** -8 * y.abs() + 2.0 ** -20 * (xs.abs() + (s32 * rs).abs()) + ATOL_TINY
        assert_elementwise(got[do:do + n], y, bound, f"residual_add segment {k} ({n} elements) scale {scale}", ("i",))
        assert (got[do:do + n] != x[do:do + n]).float().mean() > 0.5, "the add must move the segment"
        touched[do:do + n] = True
    assert torch.equal(got[~touched], x[~touched]), "elements between the segments were written"
    check_guards()


@pytest.mark.parametrize("scale", [1.0, 0.37])
def test_residual_add_per_element(sdlib, scale):
    """Three segments of 40x320, 10x640 and 3x1280 elements: the last block of each (2048 elements per block) is partial."""
    _residual_add_case(sdlib, [40 * 320, 10 * 640, 3 * 1280], [8, 24, 4096], scale, seed=3)


def test_residual_add_table_of_thirteen_and_ragged_tails(sdlib):
    """One table of thirteen entries, among them lengths that are no multiple of 8 (the element-wise tail) and one shorter
    than a vector."""
    counts = [2048, 4096 + 8, 5, 1000, 2047, 2049, 16, 8, 12345, 640, 1280, 4095, 3]
    _residual_add_case(sdlib, counts, [8 * (1 + k % 3) for k in range(13)], 0.37, seed=4)


@pytest.mark.parametrize("B,Bs,Bc", [(3, 3, 1), (4, 2, 2)])
def test_conv_in_add_per_element(sdlib, B, Bs, Bc):
    """conv_in with the addend at 32x40 (B = 3 with Bc = 1; B = 4 over latent batch 2 with Bc = 2: both modulo reads), every
    element against float64: one bf16 rounding of the sum plus the fp32 accumulation term of tests/test_ops_gpu.py's conv_in
    test (36 fp32 products, each rounded, and the bias) with one more addition."""
    g = torch.Generator().manual_seed(17 + B)
    H, W, C = 32, 40, 320
    x = torch.randn(Bs, 4, H, W, generator=g)
    w = torch.randn(C, 4, 3, 3, generator=g) / 6
    b = torch.randn(C, generator=g)
    add = r16(torch.randn(Bc, H, W, C, generator=g))
    wt = guarded_input(w.reshape(C, 36).t().contiguous(), torch.float32, label="Wt")
    out = guarded((B, H, W, C), torch.bfloat16, label="y")
    _lib.check(sdlib.sd_op_conv_in_add(stream(), P(guarded_input(x, torch.float32, label="x")), Bs,
                                       P(guarded_input(add, torch.bfloat16, label="addend")), Bc, P(wt),
                                       P(guarded_input(b, torch.float32, label="bias")), P(out), B, H, W, C))
    torch.cuda.synchronize()
    xs = torch.cat([x] * (B // Bs))
    res = torch.cat([add] * (B // Bc)).permute(0, 3, 1, 2)
    r64, m64 = conv3x3_nhwc_ref(xs, w, b, res=res)
    assert_elementwise(out, r64, linear_bound(r64, m64, 2 * 36 + 2), f"conv_in_add B={B} Bc={Bc}", NHWC)
    plain, _ = conv3x3_nhwc_ref(xs, w, b)
    assert (out.float().cpu().double() - plain).abs().mean() > 0.3, "the addend must move the output"
    check_guards()


# ---------------------------------------------------------------------------------------------------------------------
# handles: SD-1.5 widths at 32x32 latents
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def weights():
    from sonicdiffusionbayeslab_amd.weights import (UNetConfig, controlnet_config_for, make_synthetic_controlnet_state_dict,
                                                    make_synthetic_state_dict)
    cfg = UNetConfig(sample_size=32)
    cn = controlnet_config_for(cfg)
    return cfg, make_synthetic_state_dict(cfg, seed=1234), cn, make_synthetic_controlnet_state_dict(cn, seed=1234)


@pytest.fixture(scope="module")
def nets(weights):
    from sonicdiffusionbayeslab_amd.controlnet import HipControlNetModel
    from sonicdiffusionbayeslab_amd.unet import HipUNet2DConditionModel
    cfg, sd, cn, cw = weights
    old = os.environ.get("SD_DEBUG_TAPS")
    os.environ["SD_DEBUG_TAPS"] = "1"            # (the conditioning embedding is read back through the debug-tensor call)
    try:
        cnet = HipControlNetModel(cn, cw)
    finally:
        if old is None:
            del os.environ["SD_DEBUG_TAPS"]
        else:
            os.environ["SD_DEBUG_TAPS"] = old
    return HipUNet2DConditionModel(cfg, sd), HipUNet2DConditionModel(cfg, sd), cnet


def _cond(n, h, w, seed):
    return torch.rand(n, 3, 8 * h, 8 * w, generator=torch.Generator().manual_seed(seed))


def _inputs(h, w, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(1, 4, h, w, generator=g), torch.randn(1, 77, 768, generator=g), torch.randn(1, 77, 768, generator=g)


@functools.lru_cache(maxsize=None)
def _case(t, pair, h=32, w=32):
    """Inputs of one forward (latent batch 1; ``pair``: the CFG pair [negative | positive] over the same latents)."""
    lat, pe, ne = _inputs(h, w, seed=29 + int(pair))
    ctx = torch.cat([ne, pe]) if pair else pe
    return lat, ctx, _cond(1, h, w, seed=31)


_REFS = {}


def _refs(weights, t, pair, h=32, w=32):
    """The oracle's thirteen residuals and its eps with (scale 1) and without them: computed once, shared by the tests."""
    key = (t, pair, h, w)
    if key not in _REFS:
        cfg, sd, cn, cw = weights
        lat, ctx, cond = _case(t, pair, h, w)
        oc = oracle_cfg(cfg)
        lat_in = torch.cat([lat] * ctx.shape[0])
        with torch.no_grad():
            down, mid = controlnet_forward(cw, oc, lat_in, t, ctx, cond)
            _REFS[key] = (down, mid, unet_forward_with_residuals(sd, oc, lat_in, t, ctx, down, mid),
                          unet_forward_with_residuals(sd, oc, lat_in, t, ctx))
    return _REFS[key]


def test_cond_embedding_matches_oracle(weights, nets):
    """256x320 pixels (32x40 latents), Bc = 2, through sd_controlnet_set_cond_hw and read back with the debug-tensor call."""
    cfg, sd, cn, cw = weights
    cnet = nets[2]
    cond = _cond(2, 32, 40, seed=7)
    cnet.set_cond(cond)
    got = cnet.debug_cond_embedding()
    with torch.no_grad():
        ref = cond_embedding(cw, cond).permute(0, 2, 3, 1)
        rounded = cond_embedding(cw, cond, round_bf16=True).permute(0, 2, 3, 1)
    err, cs = rel_l2(got, ref), cosine(got, ref)
    print(f"conditioning embedding 256x320 Bc=2: rel-L2 {err:.3e} cos {cs:.5f} (rms {ref.pow(2).mean().sqrt().item():.3f}); "
          f"the CPU chain with bf16 rounding after every conv is {rel_l2(rounded, ref):.3e} from the fp32 oracle")
    assert tuple(got.shape) == (2, 32, 40, 320) and torch.isfinite(got).all() and err < ENC_TOL
    assert rel_l2(got[0], got[1]) > 0.1          # two different images


def _run_controlnet(cnet, lat, ctx, cond, t):
    from sonicdiffusionbayeslab_amd.controlnet import unpack_residuals
    h, w = lat.shape[2:]
    cnet.set_context(ctx.cuda(), h, w)
    cnet.set_cond(cond)
    buf = cnet.forward_residuals(lat.cuda(), ctx.shape[0], t)
    torch.cuda.synchronize()
    down, mid = unpack_residuals(buf, cnet.config, ctx.shape[0], h, w)
    return buf, [d.cpu() for d in down], mid.cpu()


@pytest.mark.parametrize("t", [981.0, 21.0])
@pytest.mark.parametrize("pair", [False, True])
def test_controlnet_forward_matches_oracle(weights, nets, t, pair):
    lat, ctx, cond = _case(t, pair)
    rd, rm, _, _ = _refs(weights, t, pair)
    _, down, mid = _run_controlnet(nets[2], lat, ctx, cond, t)
    errs = [rel_l2(a, b) for a, b in zip(down + [mid], rd + [rm])]
    print(f"ControlNet forward t={t} pair={pair}: rel-L2 of the 13 residuals " + " ".join(f"{e:.2e}" for e in errs))
    assert len(down) == 12 and all(tuple(a.shape) == tuple(b.shape) for a, b in zip(down + [mid], rd + [rm]))
    assert all(torch.isfinite(a).all() for a in down + [mid]) and max(errs) < UNET_TOL


def test_controlnet_forward_at_32x40(weights, nets):
    lat, ctx, cond = _case(499.0, False, 32, 40)
    rd, rm, _, _ = _refs(weights, 499.0, False, 32, 40)
    _, down, mid = _run_controlnet(nets[2], lat, ctx, cond, 499.0)
    errs = [rel_l2(a, b) for a, b in zip(down + [mid], rd + [rm])]
    print("ControlNet forward 32x40: rel-L2 of the 13 residuals " + " ".join(f"{e:.2e}" for e in errs))
    assert max(errs) < UNET_TOL


def _run_unet(net, cnet, lat, ctx, cond, t, scale=1.0):
    h, w = lat.shape[2:]
    ub = ctx.shape[0]
    buf, _, _ = _run_controlnet(cnet, lat, ctx, cond, t)
    net.set_deepcache(-1)
    net.set_context(ctx.cuda(), h, w)
    net.clear_control_residuals()
    off = net.forward_latents(lat.cuda(), ub, t).clone()
    net.set_control_residuals(buf, scale, ub, h, w)
    on = net.forward_latents(lat.cuda(), ub, t).clone()
    torch.cuda.synchronize()
    net.clear_control_residuals()
    return on, off


@pytest.mark.parametrize("t", [981.0, 21.0])
@pytest.mark.parametrize("pair", [False, True])
def test_unet_with_residuals_matches_oracle(weights, nets, t, pair):
    lat, ctx, cond = _case(t, pair)
    _, _, ref_on, ref_off = _refs(weights, t, pair)
    on, off = _run_unet(nets[0], nets[2], lat, ctx, cond, t)
    e_on, e_off, apart = rel_l2(on, ref_on), rel_l2(off, ref_off), rel_l2(on, off)
    print(f"UNet t={t} pair={pair}: with residuals rel-L2 {e_on:.3e} cos {cosine(on, ref_on):.5f}; without {e_off:.3e}; "
          f"with vs without {apart:.3e} (oracle {rel_l2(ref_on, ref_off):.3e})")
    assert torch.isfinite(on).all() and e_on < UNET_TOL and e_off < UNET_TOL
    assert apart > 10 * UNET_TOL


def test_unet_with_residuals_at_32x40(weights, nets):
    lat, ctx, cond = _case(499.0, False, 32, 40)
    _, _, ref_on, _ = _refs(weights, 499.0, False, 32, 40)
    on, off = _run_unet(nets[0], nets[2], lat, ctx, cond, 499.0)
    err = rel_l2(on, ref_on)
    print(f"UNet 32x40 with residuals: rel-L2 {err:.3e} cos {cosine(on, ref_on):.5f}")
    assert torch.isfinite(on).all() and err < UNET_TOL and rel_l2(on, off) > 10 * UNET_TOL


def test_identity_and_launch_accounting(weights, nets):
    cfg, sd, cn, cw = weights
    net, never, cnet = nets
    lat, pe, ne = synth_inputs(cfg, 2, seed=5)
    ctx = torch.cat([ne, pe])
    cond = _cond(2, 32, 32, seed=9)
    x = lat.cuda()
    buf, _, _ = _run_controlnet(cnet, lat, ctx, cond, 501.0)
    for n in (net, never):
        n.set_deepcache(-1)
        n.set_context(ctx.cuda())
    ref = never.forward_latents(x, 4, 501.0).clone()
    prof_never = never.forward_profiled(x, 4, 501.0)
    net.set_control_residuals(buf, 1.0, 4)
    on = net.forward_latents(x, 4, 501.0).clone()
    prof_on = net.forward_profiled(x, 4, 501.0)
    net.clear_control_residuals()
    cleared = net.forward_latents(x, 4, 501.0).clone()
    prof_cleared = net.forward_profiled(x, 4, 501.0)
    torch.cuda.synchronize()
    assert torch.equal(cleared, ref) and rel_l2(on, ref) > 10 * UNET_TOL
    launches = lambda p: {k: v["launches"] for k, v in p.items()}
    assert launches(prof_cleared) == launches(prof_never) and "residual_add" not in launches(prof_never)
    lo, ln = launches(prof_on), launches(prof_never)
    assert lo.pop("residual_add") == 1                                  # the one add launch
    # a GroupNorm that took its statistics from the producer of a tensor the variant modifies runs its own statistics pass:
    # the same GroupNorm launches (the pass is inside sd_launch_groupnorm's count of one per op) and nothing else changes,
    # except that the mid block's last conv reduces its split-K slabs itself instead of leaving them to that GroupNorm
    print(f"launches per kind, plain: {ln}\nlaunches per kind, with residuals: {lo}")
    assert {k: v for k, v in lo.items() if k != "groupnorm"} == {k: v for k, v in ln.items() if k != "groupnorm"}
    assert lo["groupnorm"] == ln["groupnorm"]
    # residuals set for another batch or size: the forward fails and says so (the handle, below the wrapper's own check)
    net.set_control_residuals(buf, 1.0, 4)
    lib, ws = net._lib, net._workspace(4)
    out = torch.empty(2, 4, 32, 32, device="cuda")
    rc = lib.sd_unet_forward_hw(net._handle, stream(), x.data_ptr(), 2, 2, 32, 32, 501.0, out.data_ptr(), net._ws_ptr(ws), ws.numel() - 256, 0, -1)
    assert rc != 0 and b"residuals were set for batch 4 at 32x32" in lib.sd_last_error()
    net.set_context(ctx[:2].cuda())
    with pytest.raises(_lib.SdHipError, match="set_control_residuals"):
        net.forward_latents(x, 2, 501.0)
    net.clear_control_residuals()


def test_diffusers_style_call_with_additional_residuals(weights, nets):
    """``down_block_additional_residuals`` / ``mid_block_additional_residual`` as NCHW floats, already scaled: the call rounds
    them to the buffer's bf16 and adds them at scale 1."""
    cfg, sd, cn, cw = weights
    net, never, cnet = nets
    lat, ctx, cond = _case(981.0, False)
    x, c = lat.cuda(), ctx.cuda()
    down, mid = cnet(x, torch.tensor(981), encoder_hidden_states=c, controlnet_cond=cond, conditioning_scale=1.0)
    a = net(x, 981, encoder_hidden_states=c, down_block_additional_residuals=down, mid_block_additional_residual=mid)[0].clone()
    none = net(x, 981, encoder_hidden_states=c)[0].clone()
    b, _ = _run_unet(net, cnet, lat, ctx, cond, 981.0)
    p = never(x, 981, encoder_hidden_states=c)[0].clone()
    torch.cuda.synchronize()
    assert torch.equal(a, b) and torch.equal(none, p) and rel_l2(a, p) > 10 * UNET_TOL
    with pytest.raises(NotImplementedError):
        net(x, 981, encoder_hidden_states=c, down_block_additional_residuals=down)


# ---------------------------------------------------------------------------------------------------------------------
# pipelines (16x16 latents, 128x128 pixels)
# ---------------------------------------------------------------------------------------------------------------------
def _sched(name, **kw):
    from sonicdiffusionbayeslab_amd.registry import schedulers_registry
    from sonicdiffusionbayeslab_amd.schedulers import PNDMConfigStub
    return schedulers_registry[name].from_config(PNDMConfigStub().config, **kw)


@pytest.fixture(scope="module")
def controlnet_dir(weights, tmp_path_factory):
    """The synthetic ControlNet as a local directory in the upstream layout (bf16: the values are on that grid)."""
    import json
    from safetensors.torch import save_file
    cfg, sd, cn, cw = weights
    d = tmp_path_factory.mktemp("controlnet")
    (d / "config.json").write_text(json.dumps({"conditioning_embedding_out_channels": list(cn.conditioning_embedding_out_channels),
                                               "controlnet_conditioning_channel_order": "rgb", "global_pool_conditions": False}))
    save_file({k: v.to(torch.bfloat16).contiguous() for k, v in cw.items()}, str(d / "diffusion_pytorch_model.safetensors"))
    return d


def _model(weights, controlnet_dir, ucfg=None, sd=None, **kw):
    from sonicdiffusionbayeslab_amd.registry import models_registry
    cfg, sd0, cn, cw = weights
    m = models_registry["stable_diffusion_model"](unet_config=ucfg or dataclasses.replace(cfg, sample_size=16),
                                                  state_dict=dict(sd0 if sd is None else sd), **kw)
    m.load_controlnet(str(controlnet_dir))
    return m


@pytest.fixture(scope="module")
def pipe(weights, controlnet_dir):
    return _model(weights, controlnet_dir).to("cuda:0")


def test_text_to_image_two_ddim_steps_and_the_guidance_window(weights, pipe):
    from oracle.pipeline import sample_loop
    from oracle.schedulers import DDIMOracle
    cfg, sd, cn, cw = weights
    cfg16 = dataclasses.replace(cfg, sample_size=16)
    oc = oracle_cfg(cfg16)
    pipe.scheduler = _sched("ddim_scheduler")
    lat, pe, ne = synth_inputs(cfg16, 1, seed=41)
    cond = _cond(1, 16, 16, seed=42)
    kw = dict(prompt_embeds=pe, negative_prompt_embeds=ne, latents=lat, num_inference_steps=2, guidance_scale=7.5, output_type="latent")
    ran = []                                                           # timesteps the ControlNet ran at, per call

    def counted(**more):
        pipe._ensure_controlnet()
        inner = pipe.controlnet.forward_residuals
        ran.append([])
        pipe.controlnet.forward_residuals = lambda lat_, ub, t, out=None: (ran[-1].append(float(t)), inner(lat_, ub, t, out))[1]
        try:
            return pipe(**more, **kw)[0]
        finally:
            del pipe.controlnet.forward_residuals
    out = counted(control_image=cond, controlnet_conditioning_scale=0.8)
    half = counted(control_image=cond, controlnet_conditioning_scale=0.8, control_guidance_end=0.5)
    zero = counted(control_image=cond, controlnet_conditioning_scale=0.0)
    plain = counted()
    ts = [float(t) for t in pipe.scheduler._timesteps_list]
    assert ran == [ts, ts[:1], [], []] and len(ts) == 2               # every step; step 0 only (step 1 ran plain); never; never
    big, _, _ = pipe(control_image=torch.nn.functional.interpolate(cond, size=(64, 64)), controlnet_conditioning_scale=0.8, **kw)
    ref = control_loop(sd, cw, oc, DDIMOracle(), pe, ne, lat, 2, 7.5, cond, 0.8)
    ref_half = control_loop(sd, cw, oc, DDIMOracle(), pe, ne, lat, 2, 7.5, cond, 0.8, 0.0, 0.5)       # step 0 conditioned, step 1 plain
    ref_plain, _, _, _ = sample_loop(sd, oc, DDIMOracle(), pe, ne, lat, 2, 7.5)
    for what, a, b in (("conditioned", out.images, ref), ("control_guidance_end=0.5", half.images, ref_half), ("plain", plain.images, ref_plain)):
        err, cs = rel_l2(a, b), cosine(a, b)
        print(f"text-to-image DDIM 2 steps, {what}: rel-L2 {err:.3e} cos {cs:.5f}")
        assert err < FREE_TOL and cs > FREE_COS
    print(f"oracle: conditioned vs plain {rel_l2(ref, ref_plain):.3e}, window vs conditioned {rel_l2(ref_half, ref):.3e}")
    assert torch.equal(zero.images, plain.images)                       # scale 0: the plain call, bit for bit
    assert rel_l2(out.images, plain.images) > FREE_TOL and not torch.equal(half.images, out.images)
    assert tuple(pipe.control_image.shape) == (1, 3, 128, 128) and not torch.equal(big.images, plain.images)     # resized to the call's size


def test_img2img_call(weights, pipe):
    """Strength 0.75 of 4 DDIM steps: three steps run (t = 501, 251, 1).  ``control_guidance_end=0.5`` over the THREE steps
    that run keeps the ControlNet on step 0 only, keep = [1, 0, 0]; a schedule computed over the full N = 4 would keep
    [1, 1, 0] for the same steps.  On the oracle the two loops are 0.21 apart in rel-L2 and the right one is 0.43 from the
    loop without a ControlNet, so the gate below (6e-2) fails for a loop that never runs the ControlNet and for one that
    counts the window over the unsliced schedule."""
    from oracle.schedulers import DDIMOracle
    from oracle.vae import VaeConfig as OC
    from sonicdiffusionbayeslab_amd.vae import VaeConfig, make_synthetic_vae_state_dict
    from sonicdiffusionbayeslab_amd.weights import control_keep
    from tests.vae_encoder_oracle import img2img_loop
    cfg, sd, cn, cw = weights
    cfg16 = dataclasses.replace(cfg, sample_size=16)
    vcfg = VaeConfig(sample_size=16)
    vsd = make_synthetic_vae_state_dict(vcfg)
    pipe.scheduler = _sched("ddim_scheduler")
    _, pe, ne = synth_inputs(cfg16, 1, seed=45)
    img = torch.rand(1, 3, 128, 128, generator=torch.Generator().manual_seed(46))
    cond = _cond(1, 16, 16, seed=47)
    kw = dict(prompt_embeds=pe, negative_prompt_embeds=ne, image=img, strength=0.75, num_inference_steps=4, guidance_scale=7.5,
              output_type="latent")
    out, _, x0s = pipe(generator=torch.Generator().manual_seed(48), control_image=cond, control_guidance_end=0.5, **kw)
    plain, _, _ = pipe(generator=torch.Generator().manual_seed(48), **kw)
    keep = control_keep(3, 0.0, 0.5)
    with controlnet_oracle(cw, cond, keep) as calls:
        ref, _, steps = img2img_loop(sd, oracle_cfg(cfg16), vsd, OC(**dataclasses.asdict(vcfg)), DDIMOracle(), pe, ne, img, 4, 0.75, 7.5,
                                     torch.Generator().manual_seed(48))
    err, cs, apart = rel_l2(out.images, ref), cosine(out.images, ref), rel_l2(out.images, plain.images)
    print(f"img2img DDIM ({steps} steps, ControlNet on the first): rel-L2 {err:.3e} cos {cs:.5f}; against the call without a control "
          f"image {apart:.3e}")
    assert keep == [1.0, 0.0, 0.0] and calls[0] == 3 == steps == len(x0s)
    assert err < FREE_TOL and cs > FREE_COS and apart > FREE_TOL


def test_lcm_distilled_unet_call(weights, controlnet_dir):
    """An LCM-distilled UNet (guidance embedding, no CFG) with the LCM scheduler: the ControlNet (no cond_proj of its own, as
    upstream passes it no timestep_cond) runs on the single batch."""
    from sonicdiffusionbayeslab_amd.weights import make_synthetic_state_dict
    cfg, sd, cn, cw = weights
    lcfg = dataclasses.replace(cfg, sample_size=16, time_cond_proj_dim=256)
    m = _model(weights, controlnet_dir, lcfg, make_synthetic_state_dict(lcfg, seed=1234)).to("cuda:0")
    m.scheduler = _sched("lcm_scheduler")
    lat, pe, _ = synth_inputs(lcfg, 2, seed=51)
    cond = _cond(2, 16, 16, seed=52)
    noise = torch.randn(1, 2, 4, 16, 16, generator=torch.Generator().manual_seed(53))
    kw = dict(prompt_embeds=pe, latents=lat, num_inference_steps=2, guidance_scale=8.0, output_type="latent", step_noise=noise.cuda())
    a, _, _ = m(control_image=cond, **kw)
    z, _, _ = m(control_image=cond, controlnet_conditioning_scale=0.0, **kw)
    p, _, _ = m(**kw)
    assert torch.isfinite(a.images).all() and torch.equal(z.images, p.images) and rel_l2(a.images, p.images) > FREE_TOL


def test_call_with_an_ip_adapter_image_prompt_alongside(weights, controlnet_dir):
    from oracle.schedulers import DDIMOracle
    from sonicdiffusionbayeslab_amd.weights import make_synthetic_ip_adapter_state_dict, to_upstream_ip_adapter
    from tests.ip_adapter_oracle import cfg_image_embeds, ip_adapter_oracle
    cfg, sd, cn, cw = weights
    cfg16 = dataclasses.replace(cfg, sample_size=16)
    icfg = dataclasses.replace(cfg16, ip_adapter_embed_dim=1024)
    ipsd = make_synthetic_ip_adapter_state_dict(icfg, seed=1234)
    f = controlnet_dir / "ip-adapter_sd15.bin"
    torch.save({g: {k: v.to(torch.bfloat16) for k, v in d.items()} for g, d in to_upstream_ip_adapter(ipsd, icfg).items()}, str(f))
    m = _model(weights, controlnet_dir)
    m.load_ip_adapter(str(f), image_encoder_folder=None)
    m = m.to("cuda:0")
    m.scheduler = _sched("ddim_scheduler")
    lat, pe, ne = synth_inputs(cfg16, 1, seed=55)
    cond, emb = _cond(1, 16, 16, seed=56), torch.randn(1, 1024, generator=torch.Generator().manual_seed(57))
    kw = dict(prompt_embeds=pe, negative_prompt_embeds=ne, latents=lat, num_inference_steps=2, guidance_scale=7.5, output_type="latent")
    out, _, _ = m(control_image=cond, ip_adapter_image_embeds=emb, **kw)
    only_ip, _, _ = m(ip_adapter_image_embeds=emb, **kw)
    w = {**sd, **ipsd}
    ref = control_loop(w, cw, oracle_cfg(cfg16), DDIMOracle(), pe, ne, lat, 2, 7.5, cond,
                       unet_ctx=lambda: ip_adapter_oracle(w, cfg_image_embeds(emb), 1.0))
    err, cs = rel_l2(out.images, ref), cosine(out.images, ref)
    print(f"text-to-image DDIM 2 steps, ControlNet + IP-Adapter: rel-L2 {err:.3e} cos {cs:.5f}")
    assert err < FREE_TOL and cs > FREE_COS and rel_l2(out.images, only_ip.images) > FREE_TOL


def test_controlnet_with_a_cond_proj_takes_a_timestep_cond(weights, nets):
    """A ControlNet whose time embedding has ``cond_proj`` (ControlNetModel.forward's ``timestep_cond``; the pipeline passes
    none): every residual against the oracle with the condition, and again after clearing it.  On the oracle the condition
    moves residuals 1 .. 12 by 0.19 - 0.37 in rel-L2 (conv_in's residual does not see the time embedding)."""
    from sonicdiffusionbayeslab_amd.controlnet import HipControlNetModel, unpack_residuals
    from sonicdiffusionbayeslab_amd.models import get_guidance_scale_embedding
    from sonicdiffusionbayeslab_amd.weights import ControlNetConfig, UNetConfig, make_synthetic_controlnet_state_dict
    cfg16 = UNetConfig(sample_size=16)
    cn = ControlNetConfig(unet=UNetConfig(sample_size=16, time_cond_proj_dim=256))
    cw = make_synthetic_controlnet_state_dict(cn, seed=1234)
    cnet = HipControlNetModel(cn, cw)
    lat, pe, _ = synth_inputs(cfg16, 1, seed=61)
    cond = _cond(1, 16, 16, seed=62)
    tc = get_guidance_scale_embedding(7.0, 256).reshape(-1)
    oc = oracle_cfg(cfg16)
    with torch.no_grad():
        ref_on = controlnet_forward(cw, oc, lat, 501.0, pe, cond, timestep_cond=tc)
        ref_off = controlnet_forward(cw, oc, lat, 501.0, pe, cond)
    cnet.set_context(pe.cuda(), 16, 16)
    cnet.set_cond(cond)
    got = {}
    for what, c in (("on", tc), ("off", None)):
        cnet.set_timestep_cond(c)
        buf = cnet.forward_residuals(lat.cuda(), 1, 501.0)
        torch.cuda.synchronize()
        down, mid = unpack_residuals(buf, cn, 1, 16, 16)
        got[what] = [d.cpu() for d in down] + [mid.cpu()]
    for what, ref in (("on", ref_on), ("off", ref_off)):
        errs = [rel_l2(a, b) for a, b in zip(got[what], ref[0] + [ref[1]])]
        print(f"ControlNet with cond_proj, condition {what}: worst residual rel-L2 {max(errs):.3e}")
        assert max(errs) < UNET_TOL
    assert min(rel_l2(a, b) for a, b in zip(got["on"][1:], got["off"][1:])) > 5 * UNET_TOL
    with pytest.raises(ValueError, match="cond_proj"):
        nets[2].set_timestep_cond(tc)                                   # a ControlNet without cond_proj refuses a condition
