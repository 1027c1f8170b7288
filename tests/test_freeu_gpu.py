"""FreeU on the GPU: the kernel of csrc/freeu.hip per element against the fp64 closed form of tests/freeu_oracle.py, the UNet
forward against the patched oracle (every factor on its own, the blocks-swapped setting, DeepCache, ControlNet, Token Merging)
and the pipelines.

Tolerances (a priori, in the style of tests/bounds.py; inputs are bf16, the reference is fp64 from the same inputs and the fp32
factors the library receives).
  skip:   ulp_bf16(ref) + C_ACC 2^-24 (H W + 8) mag + ATOL_TINY,  mag = |x| + |s - 1| 4 mean_plane|x|
          -- one output rounding; the correction is (s - 1) / (H W) times four modes, each a sum of H W terms x[m] t(m) t(n) with
          |t| <= 1, so 4 mean_plane|x| |s - 1| bounds its magnitude; every term passes through C_ACC = 6 rounded fp32 factors (the
          count csrc/freeu.hip documents: two table entries, their angle-sum combination, the multiply-add into the sum, the same
          combination on the apply side, the scale) and at most H W additions; "+ 8" covers the cross-lane and cross-wave adds.
  hidden: scaled half ulp_bf16(ref) + ATOL_TINY (one fp32 product, one rounding); unscaled half bit-identical."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from sonicdiffusionbayeslab_amd import _lib
from tests import freeu_oracle as fo
from tests.bounds import ATOL_TINY, NHWC, assert_elementwise, check_guards, forget_guards, guarded, guarded_input, ulp_bf16
from tests.util import cosine, rel_l2

UNET_TOL = 2e-2                     # tests/test_unet_gpu.py
FREE_TOL, FREE_COS = 6e-2, 0.998    # tests/test_pipeline_gpu.py
U32 = 2.0 ** -24
C_ACC = 6                           # rounded factors per term: csrc/freeu.hip, "Rounding"

#          B  H   W   C_hidden C_skip
SHAPES = [(2, 2, 2, 1280, 1280), (2, 2, 3, 1280, 1280), (2, 5, 5, 1280, 1280), (2, 10, 10, 1280, 640), (1, 9, 18, 1280, 640),
          (1, 16, 16, 1280, 1280), (2, 32, 32, 1280, 640), (3, 8, 12, 64, 32), (1, 64, 64, 64, 32)]
FACTORS = [(0.9, 1.2), (0.2, 1.6), (1.7, 0.5)]          # (s, b)
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


@pytest.fixture(scope="module")
def sdlib():
    return _lib.load()


def f32(v):
    return float(torch.tensor(v, dtype=torch.float32))


def make_inputs(B, H, W, Ch, Cs, seed=0):
    """bf16 NHWC (hidden, skip): noise on a per-plane offset and a smooth ramp, so the four filtered modes carry weight."""
    g = torch.Generator().manual_seed(seed + 1000 * H + W)
    hidden = torch.randn(B, H, W, Ch, generator=g)
    n1 = torch.arange(H, dtype=torch.float32)[None, :, None, None] / H
    n2 = torch.arange(W, dtype=torch.float32)[None, None, :, None] / W
    skip = torch.randn(B, H, W, Cs, generator=g) + torch.randn(B, 1, 1, Cs, generator=g) + \
        torch.randn(B, 1, 1, Cs, generator=g) * n1 + torch.randn(B, 1, 1, Cs, generator=g) * n2
    return hidden.to(torch.bfloat16), skip.to(torch.bfloat16)


def gpu_freeu(sdlib, hidden, skip, b, s):
    B, H, W, Ch = hidden.shape
    Cs = skip.shape[-1]
    hi, sk = guarded_input(hidden, torch.bfloat16, label="hidden"), guarded_input(skip, torch.bfloat16, label="skip")
    ho, so = guarded((B, H, W, Ch), torch.bfloat16, label="hidden_out"), guarded((B, H, W, Cs), torch.bfloat16, label="skip_out")
    _lib.check(sdlib.sd_op_freeu(stream(), P(hi), P(sk), P(ho), P(so), B, H, W, Ch, Cs, b, s), "sd_op_freeu")
    torch.cuda.synchronize()
    assert torch.equal(hi.cpu(), hidden) and torch.equal(sk.cpu(), skip)          # the inputs are never modified
    return ho.cpu(), so.cpu()


def skip_ref_bound(skip, s):
    """(fp64 reference [B, H, W, C], bound) of the filtered skip for the fp32 factor the library receives."""
    B, H, W, C = skip.shape
    x = skip.double()
    ref = fo.fourier_filter_closed(x.permute(0, 3, 1, 2), f32(s)).permute(0, 2, 3, 1)
    mag = x.abs() + abs(f32(s) - 1.0) * 4.0 * x.abs().mean(dim=(1, 2), keepdim=True)
    return ref, ulp_bf16(ref) + C_ACC * U32 * (H * W + 8) * mag + ATOL_TINY


def check_kernel(sdlib, shape, s, b, what):
    B, H, W, Ch, Cs = shape
    hidden, skip = make_inputs(*shape)
    ho, so = gpu_freeu(sdlib, hidden, skip, b, s)
    ref, bound = skip_ref_bound(skip, s)
    assert_elementwise(so, ref, bound, f"{what} skip", NHWC)
    half = Ch // 2
    href = hidden[..., :half].double() * f32(b)
    assert_elementwise(ho[..., :half], href, ulp_bf16(href) + ATOL_TINY, f"{what} hidden, scaled half", NHWC)
    assert torch.equal(ho[..., half:].view(torch.int16), hidden[..., half:].view(torch.int16)), f"{what}: the unscaled half changed"
    check_guards()


# ------------------------------------------------------------------------------------------------------------- 1. kernel
@pytest.mark.parametrize("s,b", FACTORS)
@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
def test_kernel_per_element(sdlib, shape, s, b):
    check_kernel(sdlib, shape, s, b, f"freeu {shape} s={s} b={b}")


# ----------------------------------------------------------------------------------------------------------- 2. identity
@pytest.mark.parametrize("shape", [(2, 5, 5, 1280, 1280), (3, 8, 12, 64, 32), (1, 64, 64, 64, 32)])
def test_s1_b1_is_the_identity(sdlib, shape):
    hidden, skip = make_inputs(*shape)
    ho, so = gpu_freeu(sdlib, hidden, skip, 1.0, 1.0)
    assert torch.equal(ho, hidden) and torch.equal(so, skip)
    check_guards()


# ----------------------------------------------------------------------------------------------------------- 3. patterns
@pytest.mark.parametrize("H,W", [(8, 12), (5, 7), (16, 16)])
@pytest.mark.parametrize("s", [0.2, 1.7])
def test_patterns_a_wrong_box_would_pass_on_noise(sdlib, H, W, s):
    """Channel 0 constant: times s.  Channel 1 cos(2 pi n1 / H): times (1 + s) / 2, only the -1 half of the pair is in the box.
    Channel 2 cos(2 pi (n1 / H - n2 / W)): unchanged, (-1, +1) is outside the box.  Channel 3 cos(2 pi (n1 / H + n2 / W)): times
    (1 + s) / 2.  The bf16 rounding d of the pure input (|d| <= 2^-9 for |x| <= 1) passes through the linear filter: against
    k x_bf16 the output differs by (s - 1) (P d - d / 2) at most, |P d| <= 4 max|d| over four modes -- 4.5 |s - 1| 2^-9 -- plus
    the output rounding and the kernel's own bound."""
    B, C = 2, 32
    n1 = torch.arange(H, dtype=torch.float64)[:, None].expand(H, W)
    n2 = torch.arange(W, dtype=torch.float64)[None, :].expand(H, W)
    skip = torch.randn(B, H, W, C, generator=torch.Generator().manual_seed(3)).double()
    skip[..., 0] = 3.0
    skip[..., 1] = torch.cos(2 * math.pi * n1 / H)
    skip[..., 2] = torch.cos(2 * math.pi * (n1 / H - n2 / W))
    skip[..., 3] = torch.cos(2 * math.pi * (n1 / H + n2 / W))
    skip = skip.to(torch.bfloat16)
    hidden = torch.randn(B, H, W, 32, generator=torch.Generator().manual_seed(4)).to(torch.bfloat16)
    _, so = gpu_freeu(sdlib, hidden, skip, 1.0, s)
    s32 = f32(s)
    _, kernel_bound = skip_ref_bound(skip, s)
    for ch, k, what in ((0, s32, "constant"), (1, (1 + s32) / 2, "cos(n1)"), (2, 1.0, "cos(n1 - n2)"), (3, (1 + s32) / 2, "cos(n1 + n2)")):
        want = k * skip[..., ch].double()
        leak = 0.0 if ch == 0 else 4.5 * abs(s32 - 1.0) * 2.0 ** -9          # (3.0 is on the bf16 grid: no input rounding)
        assert_elementwise(so[..., ch], want, kernel_bound[..., ch] + leak, f"{what} plane {H}x{W} s={s}", ("b", "y", "x"))
    check_guards()


# --------------------------------------------------------------------------------------------------- 4. other properties
def test_kernel_is_deterministic(sdlib):
    hidden, skip = make_inputs(2, 32, 32, 1280, 640)
    a = gpu_freeu(sdlib, hidden, skip, 1.6, 0.2)
    b = gpu_freeu(sdlib, hidden, skip, 1.6, 0.2)
    assert torch.equal(a[0].view(torch.int16), b[0].view(torch.int16)) and torch.equal(a[1].view(torch.int16), b[1].view(torch.int16))
    check_guards()


def test_the_op_refuses_by_name_and_writes_nothing(sdlib):
    def refused(shape, b, s, *names):
        B, H, W, Ch, Cs = shape
        bufs = [guarded((B, max(H, 1), W, c), torch.bfloat16, fill=1.0) for c in (Ch, Cs, Ch, Cs)]
        rc = sdlib.sd_op_freeu(stream(), *(P(t) for t in bufs), B, H, W, Ch, Cs, b, s)
        msg = sdlib.sd_last_error().decode()
        torch.cuda.synchronize()
        assert rc != 0 and all(n in msg for n in names), (rc, msg)
        assert all(bool((t == 1.0).all()) for t in bufs)
    refused((1, 8, 8, 48, 32), 1.2, 0.9, "C_hidden=48", "multiple of 32")
    refused((1, 8, 8, 64, 40), 1.2, 0.9, "C_skip=40", "multiple of 32")
    refused((1, 8, 8, 64, 16), 1.2, 0.9, "C_skip=16", "multiple of 32")
    refused((1, 1, 8, 64, 32), 1.2, 0.9, "plane 1x8")
    refused((1, 8, 1, 64, 32), 1.2, 0.9, "plane 8x1")
    refused((1, 8, 129, 64, 32), 1.2, 0.9, "plane 8x129")
    refused((1, 8, 8, 64, 32), 0.0, 0.9, "b=0", "> 0")
    refused((1, 8, 8, 64, 32), 1.2, -0.5, "s=-0.5", "> 0")
    check_guards()


# ------------------------------------------------------------------------------------------------------- 5. UNet forward
_NETS = {}


def net_of(name):
    from sonicdiffusionbayeslab_amd.unet import HipUNet2DConditionModel
    if name not in _NETS:
        cfg, sd, ocfg, heads = fo.env(name)
        _NETS[name] = HipUNet2DConditionModel(cfg, sd)
    return _NETS[name]


def gpu_forward(name, h, w, lb, ub, factors, t=fo.T_STEP):
    cfg = fo.env(name)[0]
    net = net_of(name)
    lat, ctx, _ = fo.unet_inputs(cfg, h, w, lb, ub)
    net.set_deepcache(-1)
    if factors is None:
        net.disable_freeu()
    else:
        net.set_freeu(*factors)
    try:
        net.set_context(ctx.cuda(), h, w)
        eps = net.forward_latents(lat.cuda(), ub, t).clone()
        torch.cuda.synchronize()
    finally:
        net.disable_freeu()
    return eps.cpu()


@pytest.mark.parametrize("case", fo.UNET_CASES, ids=[c[0] for c in fo.UNET_CASES])
def test_unet_forward_matches_the_patched_oracle(case):
    _, name, h, w, lb, ub, factors, floor = case
    eps = gpu_forward(name, h, w, lb, ub, factors)
    ref, plain = fo.reference(name, h, w, lb, ub, factors), fo.reference(name, h, w, lb, ub, None)
    err, moved, own = rel_l2(eps, ref), rel_l2(eps, plain), rel_l2(ref, plain)
    print(f"[freeu unet] {name} {h}x{w} batch {lb}/{ub} {factors}: rel-L2 vs the patched oracle {err:.3e}; vs the plain oracle "
          f"{moved:.3f} (oracle's own with / without {own:.3f}, floor {floor * UNET_TOL:.2f})")
    assert own > floor * UNET_TOL
    assert torch.isfinite(eps).all() and err < UNET_TOL
    assert moved > floor * UNET_TOL


def test_the_swapped_setting_is_far_and_off_is_off():
    given = gpu_forward("sd15", 16, 16, 2, 2, fo.GIVEN)
    swapped = gpu_forward("sd15", 16, 16, 2, 2, fo.SWAPPED)
    ref_sw = fo.reference("sd15", 16, 16, 2, 2, fo.SWAPPED)
    d, err = rel_l2(swapped, given), rel_l2(swapped, ref_sw)
    print(f"[freeu unet] swapped vs given {d:.3f}; swapped vs its oracle {err:.3e}")
    assert err < UNET_TOL and d > 10 * UNET_TOL
    # off is off, bit for bit, and s = b = 1 is the plain forward up to the GroupNorms' own statistics pass
    a, b = gpu_forward("sd15", 16, 16, 2, 2, None), gpu_forward("sd15", 16, 16, 2, 2, None)
    assert torch.equal(a, b)
    ones = gpu_forward("sd15", 16, 16, 2, 2, (1.0, 1.0, 1.0, 1.0))
    assert rel_l2(ones, a) < UNET_TOL


def test_the_profile_kind_counts_six_launches():
    cfg = fo.env("sd15")[0]
    net = net_of("sd15")
    lat, ctx, _ = fo.unet_inputs(cfg, 16, 16, 2, 2)
    net.set_deepcache(-1)
    net.set_freeu(*fo.GIVEN)
    try:
        net.set_context(ctx.cuda())
        prof = net.forward_profiled(lat.cuda(), 2, fo.T_STEP)
    finally:
        net.disable_freeu()
    assert prof["freeu"]["launches"] == 6 and prof["freeu"]["bytes"] > 0
    net.set_context(ctx.cuda())
    assert "freeu" not in net.forward_profiled(lat.cuda(), 2, fo.T_STEP)


# ------------------------------------------------------------------------------------------------------------ 6. DeepCache
@pytest.mark.parametrize("branch", [7, 10])
def test_deepcache_skip_steps_apply_freeu_to_the_cached_feature(branch):
    """Branch 7 = cache block 2, layer 1: the skip step runs up_blocks.1.resnets.1 on the cached output of
    up_blocks.1.attentions.0; branch 10 = cache block 3: it reaches into up block 0 as well.  Two skip steps in a row on the same
    inputs give the same eps (the cached feature stays raw), and all three steps match the oracle with its DeepCacheState."""
    from oracle.unet import DeepCacheState
    from sonicdiffusionbayeslab_amd.unet import CACHE_FULL_AND_STORE, CACHE_SKIP
    cfg, sd, ocfg, heads = fo.env("sd15")
    net = net_of("sd15")
    lat, ctx, sample = fo.unet_inputs(cfg, 16, 16, 2, 2)
    steps = ((981.0, CACHE_FULL_AND_STORE), (961.0, CACHE_SKIP), (961.0, CACHE_SKIP))
    net.set_freeu(*fo.GIVEN)
    net.set_deepcache(branch)
    try:
        net.set_context(ctx.cuda(), 16, 16)
        got = [net.forward_latents(lat.cuda(), 2, t, cache_mode=m).clone().cpu() for t, m in steps]
        torch.cuda.synchronize()
    finally:
        net.set_deepcache(-1)
        net.disable_freeu()
    assert torch.equal(got[1], got[2])
    dc = DeepCacheState(cache_interval=3, cache_branch_id=branch, enabled=True)
    plain_dc = DeepCacheState(cache_interval=3, cache_branch_id=branch, enabled=True)
    for i, (t, _) in enumerate(steps):
        dc.cur_timestep = plain_dc.cur_timestep = i
        ref = fo.unet_forward(sd, ocfg, sample, t, ctx, fo.GIVEN, dc=dc)
        plain = fo.unet_forward(sd, ocfg, sample, t, ctx, None, dc=plain_dc)
        err, moved, own = rel_l2(got[i], ref), rel_l2(got[i], plain), rel_l2(ref, plain)
        print(f"[freeu deepcache] branch {branch} step {i}: rel-L2 vs the oracle {err:.3e}; vs the oracle without FreeU {moved:.3f} "
              f"(oracle's own {own:.3f})")
        assert own > 5 * UNET_TOL                        # (tests/test_freeu_cpu.py checks the same floor with the oracle alone)
        assert torch.isfinite(got[i]).all() and err < UNET_TOL and moved > 5 * UNET_TOL


# ------------------------------------------------------------------------------------------------------------ 7. interplay
def test_with_a_controlnet_the_filter_sees_the_skips_after_the_residual_add():
    from sonicdiffusionbayeslab_amd.controlnet import HipControlNetModel
    from sonicdiffusionbayeslab_amd.weights import controlnet_config_for, make_synthetic_controlnet_state_dict
    from tests.controlnet_oracle import controlled_unet_forward
    cfg, sd, ocfg, _ = fo.env("sd15")
    net = net_of("sd15")
    cn = controlnet_config_for(cfg)
    cw = make_synthetic_controlnet_state_dict(cn, seed=1234)
    cnet = HipControlNetModel(cn, cw)
    h = w = 16
    lat, ctx, sample = fo.unet_inputs(cfg, h, w, 2, 2)
    cond = torch.rand(1, 3, 8 * h, 8 * w, generator=torch.Generator().manual_seed(31))
    cnet.set_context(ctx.cuda(), h, w)
    cnet.set_cond(cond)
    buf = cnet.forward_residuals(lat.cuda(), 2, fo.T_STEP)
    net.set_deepcache(-1)
    net.set_freeu(*fo.GIVEN)
    try:
        net.set_context(ctx.cuda(), h, w)
        net.set_control_residuals(buf, 1.0, 2, h, w)
        eps = net.forward_latents(lat.cuda(), 2, fo.T_STEP).clone().cpu()
        torch.cuda.synchronize()
    finally:
        net.clear_control_residuals()
        net.disable_freeu()
    with torch.no_grad():
        ref = controlled_unet_forward(sd, cw, ocfg, sample, fo.T_STEP, ctx, cond, 1.0, unet_ctx=lambda: fo.patched(fo.GIVEN))
        no_freeu = controlled_unet_forward(sd, cw, ocfg, sample, fo.T_STEP, ctx, cond, 1.0)
    no_control = fo.reference("sd15", h, w, 2, 2, fo.GIVEN)
    err = rel_l2(eps, ref)
    print(f"[freeu + controlnet] rel-L2 vs the combined oracle {err:.3e}; vs ControlNet alone {rel_l2(eps, no_freeu):.3f}; vs FreeU "
          f"alone {rel_l2(eps, no_control):.3f} (oracle: {rel_l2(ref, no_freeu):.3f}, {rel_l2(ref, no_control):.3f})")
    assert torch.isfinite(eps).all() and err < UNET_TOL
    assert rel_l2(ref, no_freeu) > 10 * UNET_TOL and rel_l2(eps, no_freeu) > 10 * UNET_TOL
    assert rel_l2(ref, no_control) > UNET_TOL and rel_l2(eps, no_control) > UNET_TOL


def test_with_token_merging():
    """Token Merging at ratio 0.5 on the first level and FreeU together: the library's own matchings fed to the oracle under
    both patches (tests/test_tome_gpu.py: a free-running oracle may resolve a near-tie of two similarities differently)."""
    from tests import tome_oracle as to
    cfg, sd, ocfg, heads = fo.env("sd15")
    net = net_of("sd15")
    h = w = 16
    lat, ctx, sample, choice = to.unet_inputs(cfg, h, w, 2, 2, 1)
    assert torch.equal(sample, fo.unet_inputs(cfg, h, w, 2, 2)[2])
    net.set_deepcache(-1)
    net.set_tome(0.5, 1)
    net.set_freeu(*fo.GIVEN)
    try:
        blocks = net.tome_blocks(h, w)
        net.set_context(ctx.cuda(), h, w)
        net.set_tome_choice(choice.cuda(), h, w)
        eps = net.forward_latents(lat.cuda(), 2, fo.T_STEP).clone().cpu()
        torch.cuda.synchronize()
        given, choices = [], []
        for i, b in enumerate(blocks):
            m = net.tome_matching(i, 2, h, w)
            given.append({k: m[k] for k in ("kept", "merged", "dst_idx")})
            choices.append(choice[b["choice_off"]:b["choice_off"] + (b["h"] // 2) * (b["w"] // 2)])
    finally:
        net.set_tome(0.0)
        net.disable_freeu()
    assert len(blocks) == 5
    with fo.patched(fo.GIVEN):
        ref = to.unet_forward(sd, ocfg, sample, fo.T_STEP, ctx, to.TomeRun((h, w), 0.5, 1, choices, given=given))
    tome_only = to.unet_forward(sd, ocfg, sample, fo.T_STEP, ctx, to.TomeRun((h, w), 0.5, 1, choices, given=given))
    freeu_only = fo.reference("sd15", h, w, 2, 2, fo.GIVEN)
    err = rel_l2(eps, ref)
    print(f"[freeu + tome] rel-L2 vs the combined oracle {err:.3e}; vs Token Merging alone {rel_l2(eps, tome_only):.3f}; vs FreeU "
          f"alone {rel_l2(eps, freeu_only):.3f}")
    assert torch.isfinite(eps).all() and err < UNET_TOL
    assert rel_l2(eps, tome_only) > 10 * UNET_TOL and rel_l2(eps, freeu_only) > UNET_TOL


# ---------------------------------------------------------------------------------------------------------- 8. model level
@pytest.fixture(scope="module")
def pipe():
    from sonicdiffusionbayeslab_amd.models import StableDiffusionModel
    from sonicdiffusionbayeslab_amd.registry import schedulers_registry
    cfg, sd, ocfg, _ = fo.env("sd15")
    model = StableDiffusionModel(unet_config=cfg, state_dict=dict(sd)).to("cuda:0")
    model.scheduler = schedulers_registry["ddim_scheduler"].from_config(model.scheduler.config)
    return cfg, sd, ocfg, model


def _call(model, steps=4):
    g = torch.Generator().manual_seed(29)
    lat = torch.randn((1, 4, 16, 16), generator=g)
    pe, ne = torch.randn((1, 77, 768), generator=g), torch.randn((1, 77, 768), generator=g)
    out = model(prompt_embeds=pe, negative_prompt_embeds=ne, latents=lat, num_inference_steps=steps, guidance_scale=7.5,
                output_type="latent")[0].images.float().cpu()
    return out, (lat, pe, ne)


def test_model_enable_and_disable_freeu(pipe):
    from oracle.pipeline import sample_loop
    from oracle.schedulers import DDIMOracle
    cfg, sd, ocfg, model = pipe
    plain, (lat, pe, ne) = _call(model)
    assert model.enable_freeu(*fo.GIVEN) is model
    on, _ = _call(model)
    plans = model.unet.plan_count()
    with fo.patched(fo.GIVEN), torch.no_grad():
        ref = sample_loop(sd, ocfg, DDIMOracle(), pe, ne, lat, 4, 7.5)[0]
    err, cs, moved = rel_l2(on, ref), cosine(on, ref), rel_l2(on, plain)
    print(f"[freeu model] 4-step DDIM: rel-L2 vs the oracle loop {err:.3e} cos {cs:.5f}; with / without FreeU {moved:.3f}")
    assert torch.isfinite(on).all() and moved > FREE_TOL
    assert err < FREE_TOL and cs > FREE_COS
    model.enable_freeu(*fo.SWAPPED)                      # other factors: the same plans, another result
    other, _ = _call(model)
    assert model.unet.plan_count() == plans and not torch.equal(other, on)
    model.enable_freeu(*fo.GIVEN)
    again, _ = _call(model)
    assert model.unet.plan_count() == plans and torch.equal(again, on)
    assert model.disable_freeu() is model
    off, _ = _call(model)
    assert torch.equal(off, plain)                       # a never-enabled model's result, bit for bit
