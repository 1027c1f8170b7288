"""Non-square latents (height / width per call) on the GPU: the 3x3 conv at the geometries of 512x768, 768x512 and
768x768 images, the long-row softmax of the VAE mid-block attention beyond 4096 tokens, the VAE decoder, the UNet
forward and the pipelines at 512x768 -- each against the fp32 CPU oracle (oracle/*.py: shape-generic torch ops).
Tolerances are those of the square tests they mirror (test_ops_gpu.py, test_fp8_gpu.py, test_vae_gpu.py,
test_unet_gpu.py, test_fullsize_gpu.py, test_pipeline_gpu.py)."""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from sonicdiffusionbayeslab_amd import _lib
from tests.util import cosine, oracle_cfg, rel_l2
from tests.bounds import (ATOL_TINY, U32, NHWC, assert_e4m3_codes, assert_elementwise, attention_elementwise, check_guards,
                          conv3x3_nhwc_ref, conv_gn_elementwise, device_operand, forget_guards, fp8_conv_ref,
                          fp8_gemm_ref_bound, geglu_ref_bound, gemm_bound, grouped_softmax_elementwise, guarded,
                          guarded_input, linear_bound, ln_fold_elementwise, ln_fold_ref_bound, norm_ref_bound, sample_rows,
                          softmax_rows_ref_bound, softmax_rows_elementwise, subpixel_ref, ulp_bf16,
                          xattn_elementwise)

OP_TOL = 6e-3                     # test_ops_gpu.py / test_fp8_gpu.py: one kernel, bf16 output rounding
UNET_TOL = 2e-2                   # one UNet forward
FREE_TOL, FREE_COS = 6e-2, 0.998  # free-running loops

_KEEP = []


def stream():
    return torch.cuda.current_stream().cuda_stream


def P(t):
    """The device pointer of a kernel operand or output: guarded buffers as they are, anything else copied into a
    NaN-poisoned guarded buffer (tests/bounds.py), kept alive until the test ends."""
    if t is None:
        return None
    t = device_operand(t)
    _KEEP.append(t)
    return t.data_ptr()


@pytest.fixture(autouse=True)
def _drop_keep():
    yield
    torch.cuda.synchronize()
    _KEEP.clear()
    check_guards()              # every guard of every operand and output of the test (tests/bounds.py)


def r16(t):
    return t.to(torch.bfloat16).float()


def inputs(latent_batch, h, w, seed, context_len=77, dim=768):
    g = torch.Generator().manual_seed(seed)
    lat = torch.randn((latent_batch, 4, h, w), generator=g)
    pe = torch.randn((latent_batch, context_len, dim), generator=g)
    ne = torch.randn((1, context_len, dim), generator=g).repeat(latent_batch, 1, 1)
    return lat, pe, ne


# ------------------------------------------------------------------------------------------ 3x3 conv, op level
# (B, Hin, Win, Cin, Cout, upsample, kernel): the stride-1 convs of the UNet at 512x768 (latent 64x96), 768x512 and
# 768x768 -- output widths 96, 48, 24, 12 and the portrait 96x64 -- and the fused upsamplers 24 -> 48 and 48 -> 96, with
# the kernel the selection rule assigns (sd_op_conv3x3_kernel: 1 = halo kernel, here its geometry mode; 0 = implicit
# GEMM: the 8x12 level, whose 8-row tiles would be 96 of 256 rows)
CONV_SHAPES = [
    (1, 64, 96, 320, 320, 0, 1), (1, 32, 48, 640, 640, 0, 1), (1, 16, 24, 1280, 1280, 0, 1), (1, 8, 12, 1280, 1280, 0, 0),
    (1, 96, 64, 320, 320, 0, 1), (1, 96, 96, 320, 320, 0, 1), (1, 48, 48, 640, 640, 0, 1),
    (16, 32, 48, 320, 320, 0, 1), (16, 16, 24, 640, 640, 0, 1), (16, 8, 12, 1280, 1280, 0, 0),
    (1, 32, 48, 640, 320, 1, 1), (1, 16, 24, 1280, 640, 1, 1), (16, 16, 24, 640, 640, 1, 1),
    (2, 16, 16, 320, 320, 0, 1),              # power-of-two geometry (unchanged kernel) beside the new mode
]


def _conv_ref(x, w, b, up):
    xin = F.interpolate(x, scale_factor=2.0, mode="nearest") if up else x
    return F.conv2d(xin, w, b, padding=1)


@pytest.mark.parametrize("B,H,W,Cin,Cout,up,kernel", CONV_SHAPES)
def test_conv3x3_non_square_bf16(sdlib, B, H, W, Cin, Cout, up, kernel):
    g = torch.Generator().manual_seed(B * 1000 + H * 10 + W + Cin)
    x = r16(torch.randn(B, Cin, H, W, generator=g))
    w = r16(torch.randn(Cout, Cin, 3, 3, generator=g) / math.sqrt(9 * Cin))
    b = torch.randn(Cout, generator=g)
    b2 = torch.randn(Cout, generator=g)
    ref = _conv_ref(x, w, b, up) + b2[None, :, None, None]
    Ho, Wo = ref.shape[-2:]
    r = r16(torch.randn(B, Cout, Ho, Wo, generator=g))
    ref = ref + r
    xd = x.permute(0, 2, 3, 1).contiguous().to(torch.bfloat16)
    wd = w.permute(0, 2, 3, 1).reshape(Cout, 9, Cin // 64, 64).permute(0, 2, 1, 3).contiguous().to(torch.bfloat16)
    rd = r.permute(0, 2, 3, 1).contiguous().to(torch.bfloat16)
    out = guarded((B, Ho, Wo, Cout), torch.bfloat16)
    _lib.check(sdlib.sd_op_conv3x3(stream(), P(xd), P(wd), P(b), P(b2), P(rd), P(out), B, H, W, Cin, Cout, 1, up))
    torch.cuda.synchronize()
    err = rel_l2(out.permute(0, 3, 1, 2), ref)
    kern = sdlib.sd_op_conv3x3_kernel(B * Ho * Wo, Cout, Cin, H, W, 1, up, 0)
    print(f"conv3x3 {B}x{H}x{W} up={up} Cin={Cin} Cout={Cout}: kernel {kern} rel-L2 {err:.3e}")
    assert kern == kernel and err < OP_TOL
    r64, m64 = conv3x3_nhwc_ref(x, w, b, b2, r, 1, up)
    assert_elementwise(out, r64, linear_bound(r64, m64, 9 * Cin + 3), f"conv3x3 non-square {B}x{H}x{W} up{up} {Cin}->{Cout} k{kern}", NHWC)


@pytest.mark.parametrize("B,H,W,Cin,Cout,up", [(2, 32, 48, 640, 640, 0), (1, 16, 24, 1280, 320, 1), (3, 20, 20, 128, 192, 0)])
def test_conv3x3_geometry_mode_with_split_k_and_tails(sdlib, monkeypatch, B, H, W, Cin, Cout, up):
    """The halo kernel's geometry mode (split-K at small grids, a Cout tail, a partial last tile per image: 20 rows of
    width 20 in tiles of 12) against F.conv2d, and against the implicit-GEMM kernel it replaces."""
    g = torch.Generator().manual_seed(H * W + Cin + up)
    x = r16(torch.randn(B, Cin, H, W, generator=g))
    w = r16(torch.randn(Cout, Cin, 3, 3, generator=g) / math.sqrt(9 * Cin))
    b = torch.randn(Cout, generator=g)
    ref = _conv_ref(x, w, b, up)
    Ho, Wo = ref.shape[-2:]
    xd = x.permute(0, 2, 3, 1).contiguous().to(torch.bfloat16)
    wd = w.permute(0, 2, 3, 1).reshape(Cout, 9, Cin // 64, 64).permute(0, 2, 1, 3).contiguous().to(torch.bfloat16)

    def run():
        out = guarded((B, Ho, Wo, Cout), torch.bfloat16)
        _lib.check(sdlib.sd_op_conv3x3(stream(), P(xd), P(wd), P(b), None, None, P(out), B, H, W, Cin, Cout, 1, up))
        torch.cuda.synchronize()
        return out.permute(0, 3, 1, 2).float().cpu()
    assert sdlib.sd_op_conv3x3_kernel(B * Ho * Wo, Cout, Cin, H, W, 1, up, 0) == 1
    got = run()
    monkeypatch.setenv("SD_CONV_HALO_GEN", "0")
    assert sdlib.sd_op_conv3x3_kernel(B * Ho * Wo, Cout, Cin, H, W, 1, up, 0) == 0
    other = run()
    err, diff = rel_l2(got, ref), rel_l2(got, other)
    print(f"geometry mode {B}x{H}x{W} up={up}: rel-L2 {err:.3e}, vs implicit GEMM {diff:.3e}")
    assert err < OP_TOL and diff < 2e-3
    r64, m64 = conv3x3_nhwc_ref(x, w, b, None, None, 1, up)
    bound = linear_bound(r64, m64, 9 * Cin + 1)
    assert_elementwise(got.permute(0, 2, 3, 1), r64, bound, f"conv3x3 geometry-mode {B}x{H}x{W} up{up} {Cin}->{Cout}", NHWC)
    assert_elementwise(other.permute(0, 2, 3, 1), r64, bound, f"conv3x3 implicit-gemm {B}x{H}x{W} up{up} {Cin}->{Cout}", NHWC)


def _subpixel_weights(w):
    """[Cout, Cin, 3, 3] -> [4 phases][Cout][Cin/64][4 taps][64] with the taps that read one low-res pixel summed."""
    Cout, Cin = w.shape[:2]
    rows = [[[0], [1, 2]], [[0, 1], [2]]]
    w4 = torch.zeros(4, Cout, Cin, 2, 2)
    for py in (0, 1):
        for px in (0, 1):
            for dy in (0, 1):
                for dx in (0, 1):
                    w4[py * 2 + px, :, :, dy, dx] = w[:, :, rows[py][dy]][:, :, :, rows[px][dx]].sum((2, 3))
    return w4.permute(0, 1, 3, 4, 2).reshape(4, Cout, 4, Cin // 64, 64).permute(0, 1, 3, 2, 4).contiguous()


@pytest.mark.parametrize("B,H,W,Cin,Cout", [(1, 32, 48, 640, 320), (16, 32, 48, 320, 320), (16, 16, 24, 640, 640),
                                            (1, 16, 24, 1280, 640)])
def test_conv3x3_upsample_subpixel_non_square(sdlib, B, H, W, Cin, Cout):
    """The sub-pixel upsampler (four 2x2 convs on the low-res input) at 24 -> 48 and 48 -> 96 output width."""
    g = torch.Generator().manual_seed(H + W + Cin + B)
    x = r16(torch.randn(B, Cin, H, W, generator=g))
    w = r16(torch.randn(Cout, Cin, 3, 3, generator=g) / math.sqrt(9 * Cin))
    b = torch.randn(Cout, generator=g)
    ref = _conv_ref(x, w, b, 1)
    xd = x.permute(0, 2, 3, 1).contiguous().to(torch.bfloat16)
    w4 = _subpixel_weights(w).to(torch.bfloat16)
    out = guarded((B, 2 * H, 2 * W, Cout), torch.bfloat16)
    _lib.check(sdlib.sd_op_conv3x3_upsample_subpixel(stream(), P(xd), P(w4), P(b), P(out), B, H, W, Cin, Cout))
    torch.cuda.synchronize()
    err = rel_l2(out.permute(0, 3, 1, 2), ref)
    kern = sdlib.sd_op_conv3x3_kernel(4 * B * H * W, Cout, Cin, H, W, 1, 2, 0)
    print(f"sub-pixel upsampler {B}x{H}x{W} -> {2 * H}x{2 * W}: kernel {kern} rel-L2 {err:.3e}")
    assert kern == 0 and err < OP_TOL            # (the 4-tap mode keeps power-of-two geometry: DESIGN 4b)
    r64, m64 = subpixel_ref(x, w4, b)            # from the bf16-rounded summed phase weights the kernel reads
    assert_elementwise(out, r64, linear_bound(r64, m64, 4 * Cin + 1), f"conv3x3 subpixel non-square {B}x{H}x{W} {Cin}->{Cout}", NHWC)


@pytest.mark.parametrize("B,H,W,Cin,Cout,kernel", [(1, 64, 96, 384, 320, 1), (1, 32, 48, 640, 640, 1),
                                                   (16, 16, 24, 1280, 1280, 1), (1, 96, 64, 256, 320, 1),
                                                   (16, 8, 12, 1280, 1280, 0)])
def test_conv3x3_non_square_fp8(sdlib, B, H, W, Cin, Cout, kernel):
    from oracle.fp8 import quantize_rows
    g = torch.Generator().manual_seed(B * 100 + H + W + Cin)
    xs = 8.0
    xq = (torch.randn(B, Cin, H, W, generator=g) * xs).clamp(-448, 448).to(torch.float8_e4m3fn)
    xc = xq.view(torch.uint8)
    wq, wsc = quantize_rows(torch.randn(Cout, Cin, 3, 3, generator=g) / math.sqrt(9 * Cin))
    wc = wq.clamp(-448, 448).to(torch.float8_e4m3fn).view(torch.uint8)
    b = torch.randn(Cout, generator=g)
    ref = F.conv2d(xq.float() / xs, wq * wsc[:, None, None, None], b, padding=1)
    xd = xc.permute(0, 2, 3, 1).contiguous()
    wd = wc.permute(0, 2, 3, 1).reshape(Cout, 9, Cin // 128, 128).permute(0, 2, 1, 3).contiguous()
    out = guarded((B, H, W, Cout), torch.bfloat16)
    _lib.check(sdlib.sd_op_conv3x3_fp8(stream(), P(xd), P(wd), P(wsc), xs, P(b), None, None, P(out), B, H, W, Cin, Cout,
                                       1, 0))
    torch.cuda.synchronize()
    err = rel_l2(out.permute(0, 3, 1, 2), ref)
    kern = sdlib.sd_op_conv3x3_kernel(B * H * W, Cout, Cin, H, W, 1, 0, 1)
    print(f"conv3x3 fp8 {B}x{H}x{W} Cin={Cin}: kernel {kern} rel-L2 {err:.3e}")
    assert kern == kernel and err < OP_TOL
    r64, m64, k_eff = fp8_conv_ref(xq.float() / xs, wq, wsc, b)
    assert_elementwise(out, r64, linear_bound(r64, m64, k_eff), f"conv3x3 fp8 non-square {B}x{H}x{W} {Cin}->{Cout} k{kern}", NHWC)


def test_conv3x3_kernel_report_matches_the_square_unet_shapes(sdlib):
    """sd_op_conv3x3_kernel reports the kernels the square bench plan runs (batch 16 + CFG = UNet batch 32)."""
    k = sdlib.sd_op_conv3x3_kernel
    assert k(32 * 64 * 64, 320, 320, 64, 64, 1, 0, 0) == 1          # 64x64 resnet conv: halo kernel
    assert k(32 * 8 * 8, 1280, 1280, 8, 8, 1, 0, 0) == 1            # 8x8: halo kernel, four images per tile
    assert k(32 * 64 * 64, 320, 384, 64, 64, 1, 0, 1) == 1          # fp8 resnet conv (Cin padded to 128)
    assert k(32 * 32 * 32, 320, 320, 64, 64, 2, 0, 0) == 0          # stride 2: implicit GEMM
    assert k(4 * 32 * 32 * 32, 640, 640, 32, 32, 1, 2, 0) == 2      # 32 -> 64 upsampler: 4-tap mode
    assert k(32 * 4 * 4, 1280, 1280, 4, 4, 1, 0, 0) == 0            # width 4: implicit GEMM


# ------------------------------------------------------------------------------------------ long-row softmax
@pytest.mark.parametrize("rows,cols", [(7, 6144), (3, 16384), (64, 4096)])
def test_softmax_rows_long(sdlib, rows, cols):
    g = torch.Generator().manual_seed(cols + rows)
    s = r16(torch.randn(rows, cols, generator=g) * 20)
    scale = 1 / math.sqrt(512)
    ref = torch.softmax(s * scale, dim=-1)
    d = guarded_input(s, torch.bfloat16)         # in place: the scores' own poisoned guards
    _lib.check(sdlib.sd_op_softmax_rows(stream(), d.data_ptr(), rows, cols, scale))
    torch.cuda.synchronize()
    err = rel_l2(d, ref)
    print(f"softmax {rows}x{cols}: rel-L2 {err:.3e}")
    assert torch.isfinite(d.float()).all() and err < OP_TOL
    assert torch.allclose(d.float().sum(-1).cpu(), torch.ones(rows), atol=2e-2)
    softmax_rows_elementwise(d, s, scale, f"softmax long rows {rows}x{cols}")


# ------------------------------------------------------------------------------------------ VAE decoder
def test_vae_decode_64x96_matches_oracle():
    """Latent 64x96 = 6144 mid-block tokens: chunked query rows and the long-row softmax (test_vae_gpu.py's gate)."""
    import dataclasses
    from oracle.vae import VaeConfig as OC, vae_decode
    from sonicdiffusionbayeslab_amd.vae import HipVaeDecoder, VaeConfig, make_synthetic_vae_state_dict
    cfg = VaeConfig(sample_size=64)
    sd = make_synthetic_vae_state_dict(cfg)
    dec = HipVaeDecoder(cfg, sd)
    lat = torch.randn(1, 4, 64, 96, generator=torch.Generator().manual_seed(3))
    inv = 1.0 / cfg.scaling_factor
    got = dec.decode(lat.cuda(), inv)
    torch.cuda.synchronize()
    with torch.no_grad():
        ref = vae_decode(sd, OC(**dataclasses.asdict(cfg)), lat * inv)
    err, cs = rel_l2(got, ref), cosine(got, ref)
    print(f"VAE decode 64x96 -> 512x768: rel-L2 {err:.3e} cos {cs:.5f}")
    assert got.shape == (1, 3, 512, 768) and torch.isfinite(got).all()
    assert err < 2e-2 and cs > 0.999


# ------------------------------------------------------------------------------------------ UNet forward
@pytest.fixture(scope="module")
def small():
    from sonicdiffusionbayeslab_amd.unet import HipUNet2DConditionModel
    from sonicdiffusionbayeslab_amd.weights import UNetConfig, make_synthetic_state_dict
    cfg = UNetConfig(sample_size=16)
    sd = make_synthetic_state_dict(cfg, seed=1234)
    return cfg, sd, HipUNet2DConditionModel(cfg, sd)


@pytest.mark.parametrize("h,w", [(16, 24), (24, 16)])
@pytest.mark.parametrize("t", [981.0, 21.0])
def test_small_unet_non_square_matches_oracle(small, h, w, t):
    from oracle.unet import unet_forward
    cfg, sd, net = small
    lat, pe, ne = inputs(2, h, w, seed=int(t) + h)
    ctx = torch.cat([ne, pe])
    with torch.no_grad():
        ref = unet_forward(sd, oracle_cfg(cfg), torch.cat([lat, lat]), t, ctx)
    net.set_deepcache(-1)
    net.set_context(ctx.cuda(), h, w)
    eps = net.forward_latents(lat.cuda(), 4, t)
    torch.cuda.synchronize()
    err = rel_l2(eps, ref)
    print(f"small UNet {h}x{w} t={t}: rel-L2 {err:.3e} cos {cosine(eps, ref):.5f}")
    assert eps.shape == (4, 4, h, w) and torch.isfinite(eps).all() and err < UNET_TOL


@pytest.fixture(scope="module")
def sd15():
    from sonicdiffusionbayeslab_amd.weights import UNetConfig, make_synthetic_state_dict
    cfg = UNetConfig(sample_size=64)
    return cfg, make_synthetic_state_dict(cfg, seed=1234)


def test_sd15_unet_64x96_then_64x64_on_one_handle(sd15):
    """One CFG forward at 64x96 against the oracle; then 64x64 on the SAME handle is bitwise a fresh handle's."""
    from oracle.unet import unet_forward
    from sonicdiffusionbayeslab_amd.unet import HipUNet2DConditionModel
    cfg, sd = sd15
    net = HipUNet2DConditionModel(cfg, sd)
    lat, pe, ne = inputs(1, 64, 96, seed=5)
    ctx = torch.cat([ne, pe])
    net.set_context(ctx.cuda(), 64, 96)
    eps = net.forward_latents(lat.cuda(), 2, 981.0).cpu()
    with torch.no_grad():
        ref = unet_forward(sd, oracle_cfg(cfg), torch.cat([lat, lat]), 981.0, ctx)
    err = rel_l2(eps, ref)
    print(f"SD-1.5 UNet 64x96 t=981: rel-L2 {err:.3e} cos {cosine(eps, ref):.5f}")
    assert eps.shape == (2, 4, 64, 96) and torch.isfinite(eps).all() and err < UNET_TOL

    sq, _, _ = inputs(1, 64, 64, seed=6)
    net.set_context(ctx.cuda())
    after = net.forward_latents(sq.cuda(), 2, 501.0).cpu()
    del net
    fresh = HipUNet2DConditionModel(cfg, sd)
    fresh.set_context(ctx.cuda())
    base = fresh.forward_latents(sq.cuda(), 2, 501.0).cpu()
    assert torch.equal(after, base)


# ------------------------------------------------------------------------------------------ pipelines
@pytest.fixture(scope="module")
def pipe(sd15):
    from sonicdiffusionbayeslab_amd.models import StableDiffusionModel
    cfg, sd = sd15
    return StableDiffusionModel(unet_config=cfg, state_dict=dict(sd)).to("cuda:0")


def _ddim(model):
    from sonicdiffusionbayeslab_amd.registry import schedulers_registry
    from sonicdiffusionbayeslab_amd.schedulers import PNDMConfigStub
    model.scheduler = schedulers_registry["ddim_scheduler"].from_config(PNDMConfigStub().config)


def test_pipeline_512x768_ddim_and_deepcache(sd15, pipe):
    from oracle.pipeline import sample_loop
    from oracle.schedulers import DDIMOracle
    from oracle.unet import DeepCacheState
    from sonicdiffusionbayeslab_amd.deepcache import DeepCacheSDHelper
    cfg, sd = sd15
    lat, pe, ne = inputs(2, 64, 96, seed=41)
    _ddim(pipe)
    out, secs, _ = pipe(prompt_embeds=pe, negative_prompt_embeds=ne, latents=lat, num_inference_steps=3, guidance_scale=7.5,
                        output_type="latent", height=512, width=768)
    ref, _, _, _ = sample_loop(sd, oracle_cfg(cfg), DDIMOracle(), pe, ne, lat, 3, 7.5)
    err, cs = rel_l2(out.images, ref), cosine(out.images, ref)
    print(f"DDIM 3 steps 512x768 batch 2: rel-L2 {err:.3e} cos {cs:.5f}, loop {secs * 1e3:.1f} ms")
    assert out.images.shape == (2, 4, 64, 96) and err < FREE_TOL and cs > FREE_COS

    helper = DeepCacheSDHelper(pipe=pipe)
    helper.set_params(cache_interval=3, cache_branch_id=0)
    helper.enable()
    try:
        out, _, _ = pipe(prompt_embeds=pe, negative_prompt_embeds=ne, latents=lat, num_inference_steps=3,
                         guidance_scale=7.5, output_type="latent", height=512, width=768)
    finally:
        helper.disable()
    dc = DeepCacheState(cache_interval=3, cache_branch_id=0, enabled=True)
    ref, _, _, _ = sample_loop(sd, oracle_cfg(cfg), DDIMOracle(), pe, ne, lat, 3, 7.5, deepcache=dc)
    err, cs = rel_l2(out.images, ref), cosine(out.images, ref)
    print(f"DDIM 3 steps + DeepCache N=3 512x768: rel-L2 {err:.3e} cos {cs:.5f}")
    assert err < FREE_TOL and cs > FREE_COS


def test_pipeline_512x768_pt_output(pipe):
    _ddim(pipe)
    g = torch.Generator().manual_seed(29)
    out, _, x0s = pipe(["a photo of a cat", "a dog"], num_inference_steps=1, guidance_scale=7.5, generator=g,
                       output_type="pt", height=512, width=768)
    assert out.images.shape == (2, 3, 512, 768)
    assert float(out.images.min()) >= 0 and float(out.images.max()) <= 1
    assert len(x0s) == 1 and x0s[0].shape == (1, 3, 512, 768)


def test_skip_timesteps_pipeline_768x512(sd15):
    from oracle.pipeline import sample_loop_skip
    from oracle.schedulers import DDIMOracle
    from sonicdiffusionbayeslab_amd.registry import models_registry
    cfg, sd = sd15
    model = models_registry["stable_diffusion_model_skip_timesteps"](unet_config=cfg, state_dict=dict(sd)).to("cuda:0")
    _ddim(model)
    lat, pe, ne = inputs(1, 96, 64, seed=47)
    out, _, _ = model(prompt_embeds=pe, negative_prompt_embeds=ne, latents=lat, guidance_scale=7.5, num_inference_steps=3,
                      skip_timesteps=[1], output_type="latent", height=768, width=512)
    ref, _, used = sample_loop_skip(sd, oracle_cfg(cfg), DDIMOracle(), pe, ne, lat, 3, [1], 7.5)
    err, cs = rel_l2(out.images, ref), cosine(out.images, ref)
    print(f"skip [1] of 3, 768x512: rel-L2 {err:.3e} cos {cs:.5f}")
    assert out.images.shape == (1, 4, 96, 64) and len(used) == 2 and err < FREE_TOL and cs > FREE_COS


def test_fp8_lcm_512x768(sd15):
    """fp8 weights, LCM 2 steps without CFG at 512x768; the scales come from the pipeline's fixed 64x64 calibration.
    Against the unquantised oracle: the fp8 scheme's own distance from it dominates (test_fp8_gpu.py)."""
    from oracle.pipeline import sample_loop
    from oracle.schedulers import LCMOracle
    from sonicdiffusionbayeslab_amd.models import StableDiffusionModel
    from sonicdiffusionbayeslab_amd.registry import schedulers_registry
    from sonicdiffusionbayeslab_amd.schedulers import PNDMConfigStub
    cfg, sd = sd15
    model = StableDiffusionModel(unet_config=cfg, state_dict=dict(sd), weight_dtype="fp8").to("cuda:0")
    model.scheduler = schedulers_registry["lcm_scheduler"].from_config(PNDMConfigStub().config)
    lat, pe, _ = inputs(2, 64, 96, seed=17)
    noise = torch.randn(1, 2, 4, 64, 96, generator=torch.Generator().manual_seed(8))
    out, _, _ = model(prompt_embeds=pe, latents=lat, num_inference_steps=2, guidance_scale=0.0, output_type="latent",
                      step_noise=noise.cuda(), height=512, width=768)
    assert "calibrated" in model.weights_source
    ref, _, _, _ = sample_loop(sd, oracle_cfg(cfg), LCMOracle(), pe, None, lat, 2, 0.0, lcm_noise=noise)
    err, cs = rel_l2(out.images, ref), cosine(out.images, ref)
    print(f"LCM 2 steps fp8 512x768: vs unquantised oracle rel-L2 {err:.3e} cos {cs:.5f}")
    assert out.images.shape == (2, 4, 64, 96) and torch.isfinite(out.images).all()
    assert err < 1.2e-1 and cs > 0.995          # measured 4.5e-2 / 0.9990 (test_fp8_gpu.py's loop gate: 1.2e-1)
