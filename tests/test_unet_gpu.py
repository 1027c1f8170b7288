"""Whole-UNet parity: libsdhip forward (bf16 storage, fp32 accumulate) vs the fp32 CPU oracle on
identical seeded SD-1.5-width weights.  Tolerance: rel-L2 <= 2e-2 per forward (bf16 has 8
significand bits: ~4e-3 per rounding, compounded over ~60 sequential normalised layers)."""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.util import cosine, oracle_cfg, rel_l2, synth_inputs

UNET_TOL = 2e-2
OUTLIER_TOL = 3e-2        # outlier-channel weights (measured 1.65e-2, round 4)


@pytest.fixture(scope="module")
def small_unet():
    from sonicdiffusionbayeslab_amd.unet import HipUNet2DConditionModel
    from sonicdiffusionbayeslab_amd.weights import UNetConfig, make_synthetic_state_dict
    os.environ["SD_DEBUG_TAPS"] = "1"
    cfg = UNetConfig(sample_size=16)
    sd = make_synthetic_state_dict(cfg, seed=1234)
    net = HipUNet2DConditionModel(cfg, sd)
    os.environ.pop("SD_DEBUG_TAPS")
    return cfg, sd, net


@pytest.mark.parametrize("t", [981.0, 21.0])
def test_unet_forward_matches_oracle(small_unet, t):
    from oracle.unet import unet_forward
    cfg, sd, net = small_unet
    lat, pe, ne = synth_inputs(cfg, 1)
    ctx = torch.cat([ne, pe])
    taps = {}
    with torch.no_grad():
        ref = unet_forward(sd, oracle_cfg(cfg), torch.cat([lat, lat]), t, ctx, taps=taps)
    net.set_context(ctx.cuda())
    eps = net.forward_latents(lat.cuda(), 2, t)     # CFG duplication fused into conv_in
    torch.cuda.synchronize()
    report = []
    for name, rt in taps.items():
        got = net.debug_tensor(name, 2, rt.numel()).view(rt.shape[0], rt.shape[2], rt.shape[3], rt.shape[1])
        report.append((name, rel_l2(got.permute(0, 3, 1, 2), rt)))
    err = rel_l2(eps, ref)
    print("taps:", report, "final:", err, "cos:", cosine(eps, ref))
    assert torch.isfinite(eps).all()
    assert err < UNET_TOL, report


def test_unet_diffusers_style_call(small_unet):
    """`unet(latent_model_input, t, encoder_hidden_states=...)[0]` of src/models.py:227-235."""
    cfg, sd, net = small_unet
    lat, pe, ne = synth_inputs(cfg, 2, seed=3)
    ctx = torch.cat([ne, pe]).cuda()
    x = torch.cat([lat, lat]).cuda()
    a = net(x, torch.tensor(501), encoder_hidden_states=ctx, return_dict=False)[0]
    net.set_context(ctx)
    b = net.forward_latents(lat.cuda(), 4, 501.0)
    torch.cuda.synchronize()
    assert torch.equal(a, b)           # same kernels, same order: bit-identical


def test_unet_forward_is_bitwise_reproducible_and_batch_consistent(small_unet):
    """Split-K is a fixed-order slab reduction (no atomics), so repeated forwards are bit-identical; and samples
    are independent (per-sample GroupNorm/LayerNorm/attention), so a sample's result does not depend on its
    neighbours beyond the split-K factors the batch size selects (shard-size independence)."""
    cfg, sd, net = small_unet
    lat, pe, ne = synth_inputs(cfg, 4, seed=7)
    ctx = torch.cat([ne, pe])
    net.set_context(ctx.cuda())
    a = net.forward_latents(lat.cuda(), 8, 501.0).clone()
    b = net.forward_latents(lat.cuda(), 8, 501.0).clone()
    assert torch.equal(a, b)
    # the same four samples evaluated two at a time
    halves = []
    for s in (slice(0, 2), slice(2, 4)):
        net.set_context(torch.cat([ne[s], pe[s]]).cuda())
        halves.append(net.forward_latents(lat[s].cuda(), 4, 501.0).clone())
    un = torch.cat([halves[0][:2], halves[1][:2]])
    co = torch.cat([halves[0][2:], halves[1][2:]])
    ref = torch.cat([un, co])
    assert rel_l2(a, ref) < 2e-3          # different split-K factors reassociate fp32 sums, nothing more


def _fused_groupnorms(net, lat, ub):
    """GroupNorm launches of one forward that finish their producer's deferred split-K reduce (op_times: K column > 0)."""
    import ctypes as C
    from sonicdiffusionbayeslab_amd import _lib
    out = torch.empty(ub, 4, lat.shape[2], lat.shape[3], device="cuda")
    ws = net._workspace(ub)
    buf = C.create_string_buffer(1 << 20)
    n = net._lib.sd_unet_forward_op_times(net._handle, _lib.current_stream(), lat.data_ptr(), lat.shape[0], ub, 501.0, out.data_ptr(),
                                          net._ws_ptr(ws), ws.numel() - 256, 0, net.cache_branch_id, buf, len(buf))
    assert n > 0
    rows = [l.split() for l in buf.value.decode().splitlines()]
    gn = [r for r in rows if int(r[1]) == 3]
    return sum(int(r[4]) > 0 for r in gn), len(gn)


def test_deferred_splitk_reduce_in_the_single_launch_groupnorm_is_bit_identical(small_unet):
    """At the 8x8 / 16x16 levels the plan hands the fp32 partial slabs of a split-K conv / GEMM to the single-launch GroupNorm
    that reads its output first (csrc/plan.hip fuse_deferred_reduce: resnet conv1 -> norm2, conv2 / proj_out / downsampler ->
    the next block's norm1, incl. the up path's channel concat): same sums in the same order, one launch instead of two.  A second
    handle built with SD_GN_SLAB=0 (conv + splitk_reduce, then the GroupNorm) must give the same bits."""
    from sonicdiffusionbayeslab_amd.unet import HipUNet2DConditionModel
    cfg, sd, net = small_unet
    lat, pe, ne = synth_inputs(cfg, 2, seed=5)
    ctx = torch.cat([ne, pe]).cuda()
    net.set_context(ctx)
    a = net.forward_latents(lat.cuda(), 4, 501.0).clone()
    fused, total = _fused_groupnorms(net, lat.cuda(), 4)
    assert fused >= 8, (fused, total)                  # the pass found its pairs (every resnet below the top level has two)
    os.environ["SD_GN_SLAB"] = "0"
    try:
        plain = HipUNet2DConditionModel(cfg, sd)
        plain.set_context(ctx)
        b = plain.forward_latents(lat.cuda(), 4, 501.0).clone()
        assert _fused_groupnorms(plain, lat.cuda(), 4)[0] == 0
    finally:
        del os.environ["SD_GN_SLAB"]
    assert torch.isfinite(a).all()
    assert torch.equal(a, b)


def test_cfg_prefix_deduplication_matches_explicitly_duplicated_latents(small_unet):
    """A CFG forward (UNet batch = 2 x latent batch: `torch.cat([latents] * 2)` of src/models.py:222) runs everything before
    the first prompt cross-attention once per latent and copies it to both halves; handing the library the duplicated
    latents as an ordinary batch (latent batch == UNet batch: no de-duplication) must give the same noise prediction up
    to the reassociation of fp32 partial sums that a different batch size selects."""
    cfg, sd, net = small_unet
    lat, pe, ne = synth_inputs(cfg, 3, seed=11)
    net.set_context(torch.cat([ne, pe]).cuda())
    dedup = net.forward_latents(lat.cuda(), 6, 741.0).clone()
    plain = net.forward_latents(torch.cat([lat, lat]).cuda(), 6, 741.0).clone()
    assert torch.isfinite(dedup).all()
    assert not torch.equal(dedup[:3], dedup[3:])          # the halves differ (different prompts) ...
    assert rel_l2(dedup, plain) < 2e-3                    # ... and agree with the computation done twice


def test_unet_forward_with_outlier_channels_matches_oracle():
    """The synthetic N(0, 1/fan_in) weights have no outlier channels; a trained SD-1.5 has (a few channels of the residual stream
    run at 10-30x the rest, LayerNorm gains far from 1, a BOS key every query scores high).  The three weight-space folds are
    where that could hurt: the bf16-rounded merged  Wpo . W2  (ff.net.2 + proj_out as one GEMM), the LayerNorm fold
    (W * gamma rounded to bf16, one-pass variance from row partials) and the prompt fold  A_h = scale Wq^T K^T.  Here every
    transformer block gets outlier rows / gains / offsets in exactly those tensors, and the forward is compared with the
    fp32 oracle running the UNFOLDED arithmetic on the same weights."""
    from oracle.unet import unet_forward
    from sonicdiffusionbayeslab_amd.unet import HipUNet2DConditionModel
    from sonicdiffusionbayeslab_amd.weights import UNetConfig, make_synthetic_state_dict
    cfg = UNetConfig(sample_size=16)
    sd = {k: v.clone() for k, v in make_synthetic_state_dict(cfg, seed=1234).items()}
    g = torch.Generator().manual_seed(5)
    touched = 0
    for k, w in sd.items():
        if k.endswith("ff.net.2.weight") or k.endswith("attn1.to_out.0.weight"):
            rows = torch.randperm(w.shape[0], generator=g)[:3]
            w[rows] *= 12.0                              # three outlier channels written into the residual stream
            touched += 1
        elif ".attentions." in k and k.endswith("proj_out.weight"):
            cols = torch.randperm(w.shape[1], generator=g)[:3]
            w[:, cols] *= 4.0
            touched += 1
        elif "transformer_blocks" in k and k.endswith(("norm1.weight", "norm2.weight", "norm3.weight")):
            idx = torch.randperm(w.shape[0], generator=g)[:6]
            w[idx] *= torch.tensor([6.0, 6.0, 0.1, 0.1, 3.0, 3.0])
            touched += 1
        elif "transformer_blocks" in k and k.endswith(("norm1.bias", "norm2.bias", "norm3.bias")):
            w += 0.3 * torch.randn(w.shape, generator=g)
            touched += 1
        elif k.endswith("attn2.to_q.weight") or k.endswith("attn2.to_k.weight"):
            rows = torch.randperm(w.shape[0], generator=g)[:4]
            w[rows] *= 5.0                               # a few head dimensions dominate the prompt logits
            touched += 1
    assert touched >= 10 * 16
    net = HipUNet2DConditionModel(cfg, sd)
    lat, pe, ne = synth_inputs(cfg, 1, seed=9)
    pe[:, 0] *= 4.0                                      # a BOS-like key
    ne[:, 0] *= 4.0
    ctx = torch.cat([ne, pe])
    with torch.no_grad():
        ref = unet_forward(sd, oracle_cfg(cfg), torch.cat([lat, lat]), 501.0, ctx)
    net.set_context(ctx.cuda())
    eps = net.forward_latents(lat.cuda(), 2, 501.0)
    torch.cuda.synchronize()
    err, cs = rel_l2(eps, ref), cosine(eps, ref)
    print(f"UNet forward with outlier channels / gains / BOS key: rel-L2 {err:.3e} cosine {cs:.5f}")
    assert torch.isfinite(eps).all()
    assert err < OUTLIER_TOL and cs > 0.999
