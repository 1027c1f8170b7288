"""Stable Diffusion 2.x on the GPU: head-dim-64 attention per element, the full-width SD 2 UNet (5 / 10 / 20 / 20 heads, 1024-wide
context, Linear projections) at 16x16 latents against tests/sd2_oracle.py, DeepCache, ControlNet, fp8, the gelu text tower
against the transformers golden, and free-running v-prediction loops.  Gates are the project's own for the same depth and
rounding: test_attention's (test_ops_gpu.py), UNET_TOL (test_unet_gpu.py), TOL (test_clip_gpu.py), FREE_TOL / FREE_COS
(test_pipeline_gpu.py), FWD_TOL (test_fp8_gpu.py)."""
import dataclasses
import json
import math
import os

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from sonicdiffusionbayeslab_amd import _lib
from tests import sched_ref as R
from tests.bounds import attention_elementwise, check_guards, forget_guards, guarded, guarded_input
from tests.util import CLIP_TEXTS, cosine, rel_l2, synth_inputs, synthetic_clip_vocab

UNET_TOL = 2e-2                     # tests/test_unet_gpu.py
CLIP_TOL = 1.5e-2                   # tests/test_clip_gpu.py (TOL)
FREE_TOL, FREE_COS = 6e-2, 0.998    # tests/test_pipeline_gpu.py
FWD_TOL = 1.5e-1                    # tests/test_fp8_gpu.py
PIPE_MIN_KEYS = 192                 # attn_pipe64_kernel: key counts that are multiples of 64, from its ring's three tiles on
# SD_ATTN_PIPE64 (read per call): None = the library's dispatch, "0" = attn_kernel<64>, "ones" / "valu" = attn_pipe64_kernel with
# the denominator on a third O^T tile / summed on the VALU.  Key counts the pipelined kernel does not take run attn_kernel<64>.
KERNELS = [None, "0", "ones", "valu"]
GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "clip_gelu_golden.json")

_KEEP = []


def stream():
    return torch.cuda.current_stream().cuda_stream


def r16(t):
    return t.to(torch.bfloat16).float()


def P(t):
    _KEEP.append(t)
    return t.data_ptr()


@pytest.fixture(autouse=True)
def _drop_keep():
    yield
    torch.cuda.synchronize()
    _KEEP.clear()
    forget_guards()


# ------------------------------------------------------------------------------------------------ attention, d = 64
@pytest.fixture
def pick(monkeypatch):
    def set_kernel(kernel):
        if kernel is None:
            monkeypatch.delenv("SD_ATTN_PIPE64", raising=False)
        else:
            monkeypatch.setenv("SD_ATTN_PIPE64", kernel)
    return set_kernel


def _attention(sdlib, q, k, v, heads, D):
    """sd_op_attention on guarded operands, K | V side by side as the fused projections write them."""
    B, Nq, C = q.shape
    Nk = k.shape[1]
    kv = guarded_input(torch.cat([k, v], dim=-1).contiguous(), torch.bfloat16)
    out = guarded((B, Nq, C), torch.bfloat16)
    kvp = P(kv)
    _lib.check(sdlib.sd_op_attention(stream(), P(guarded_input(q, torch.bfloat16)), C, kvp, 2 * C, kvp + 2 * C, 2 * C, P(out), C, B,
                                     heads, Nq, Nk, D, 1.0 / math.sqrt(D)))
    torch.cuda.synchronize()
    check_guards()
    return out


def _sdpa(q, k, v, heads, D):
    B, Nq, C = q.shape
    qh, kh, vh = (t.view(B, -1, heads, D).transpose(1, 2) for t in (q, k, v))
    return F.scaled_dot_product_attention(qh, kh, vh).transpose(1, 2).reshape(B, Nq, C)


D64_SHAPES = [
    (2, 5, 256, 77, False),                 # prompt cross-attention at the 5-head level
    (1, 5, 300, 300, True),                 # ragged tiles + a spiked late key (the online-max rescale)
    (2, 20, 4, 4, False),                   # the 2x2 level of a 16x16 latent: one partial tile, 20 heads
    (1, 10, 144, 144, False),               # 12x12: the 10-head level of a 768-pixel image's deepest attention
    (1, 5, 256, PIPE_MIN_KEYS, False),      # the pipelined kernel's minimum: three tiles, no steady-state pair
    (1, 5, 200, 320, True),                 # ragged queries (the last workgroup's waves past Nq), odd tile count
    (2, 10, 1024, 1024, True),              # the SD 2 32x32 self-attention shape, a spiked key in the last tile
    (1, 5, 4096, 4096, False),              # the SD 2 64x64 self-attention shape
]


def _takes(kernel, Nk):
    """Forcing a pipelined variant changes nothing at key counts it does not take: those combinations are not cases."""
    return kernel in (None, "0") or (Nk % 64 == 0 and Nk >= PIPE_MIN_KEYS)


def _kid(k):
    return "dispatch" if k is None else "general" if k == "0" else k


@pytest.mark.parametrize("kernel,B,heads,Nq,Nk,spike", [(k, *s) for s in D64_SHAPES for k in KERNELS if _takes(k, s[3])],
                         ids=lambda v: _kid(v) if v is None or isinstance(v, str) else str(v))
def test_attention_d64(sdlib, pick, kernel, B, heads, Nq, Nk, spike):
    D = 64
    pick(kernel)
    g = torch.Generator().manual_seed(Nq + 64 * Nk + heads)
    C = heads * D
    q = r16(torch.randn(B, Nq, C, generator=g))
    k = r16(torch.randn(B, Nk, C, generator=g))
    v = r16(torch.randn(B, Nk, C, generator=g))
    if spike:
        k[:, Nk - 3] = k[:, Nk - 3] * 6
    ref = _sdpa(q, k, v, heads, D)
    out = _attention(sdlib, q, k, v, heads, D)
    err = rel_l2(out, ref)
    print(f"attention d64 [{kernel}] B={B} heads={heads} {Nq}x{Nk} spike={spike}: rel-L2 {err:.3e}")
    assert err < 1e-2        # P is rounded to bf16 before PV
    attention_elementwise(out, q, k, v, heads, D, f"attention B={B} {Nq}x{Nk} d64")


DOMINANT = [(77, ((5, 13.0), (41, 26.0), (76, 39.0))),      # the prompt shape: both lane halves (bits 2, 3 of the key index)
            (512, ((5, 13.0), (296, 26.0), (509, 39.0)))]   # a multiple of 64: eight tiles


@pytest.mark.parametrize("kernel,Nk,spikes", [(k, *d) for d in DOMINANT for k in KERNELS if _takes(k, d[0])],
                         ids=lambda v: _kid(v) if v is None or isinstance(v, str) else str(v) if isinstance(v, int) else "spikes")
def test_attention_d64_survives_dominant_keys_in_either_lane_half(sdlib, pick, kernel, Nk, spikes):
    """The construction of test_ops_gpu.py::_dominant_key_case at d = 64: dominant keys at early / middle / last positions,
    each >= 150 log2 units above the maximum before it.  Finite, and rel-L2 <= 1e-2 against fp32 SDPA.  At Nk = 512 the
    pipelined kernel's stale reference has to move three times, by far more than its 2^8 threshold."""
    from tests.test_ops_gpu import _dominant_key_case
    pick(kernel)
    D, B, heads, Nq = 64, 1, 5, 256
    g = torch.Generator().manual_seed(64000 + Nk)
    q, k, v = _dominant_key_case(g, B, heads, D, Nq, Nk, spikes)
    qh, kh = (t.view(B, -1, heads, D).transpose(1, 2) for t in (q, k))
    s = (qh @ kh.transpose(-1, -2)) / math.sqrt(D) * 1.4426950408889634
    for pos, _ in spikes:
        assert (s[..., pos] - s[..., :pos].amax(-1)).min() > 150.0
    for bit in (2, 3):      # the accumulator rows one lane of a query's lane pair owns: both values of bits 2 and 3 of the key index
        assert {(p >> bit) & 1 for p, _ in spikes} == {0, 1}
    ref = _sdpa(q, k, v, heads, D)
    out = _attention(sdlib, q, k, v, heads, D)
    assert torch.isfinite(out.float()).all()
    err = rel_l2(out, ref)
    print(f"attention d64 dominant keys Nk={Nk}: rel-L2 {err:.3e}")
    assert err <= 1e-2
    attention_elementwise(out, q, k, v, heads, D, f"attention dominant keys d64 Nk={Nk}")


@pytest.mark.parametrize("kernel", ["ones", "valu"])
@pytest.mark.parametrize("Nk,spikes", [(512, ((70, 6.0), (300, 14.0), (509, 40.0))), (1024, ((5, 30.0), (640, 3.0))),
                                       (256, ((250, 25.0),))])
def test_attention_pipe64_moves_its_stale_reference(sdlib, pick, kernel, Nk, spikes):
    """test_ops_gpu.py::test_attention_pipelined_kernel_moves_its_stale_reference at d = 64: keys scaled up mid-sequence, in
    the second tile and in the last one, so that the reference moves (and O, and the VALU denominator, are rescaled) several
    times per query, by a few to hundreds of log2 units, and probabilities up to 2^8 occur between moves."""
    pick(kernel)
    g = torch.Generator().manual_seed(Nk)
    B, heads, D, Nq = 1, 5, 64, 256
    C = heads * D
    q = r16(torch.randn(B, Nq, C, generator=g))
    k = r16(torch.randn(B, Nk, C, generator=g))
    v = r16(torch.randn(B, Nk, C, generator=g))
    for pos, f in spikes:
        k[:, pos] = r16(k[:, pos] * f)
    ref = _sdpa(q, k, v, heads, D)
    out = _attention(sdlib, q, k, v, heads, D)
    assert torch.isfinite(out.float()).all()
    err = rel_l2(out, ref)
    print(f"attention d64 [{kernel}] stale reference Nk={Nk}: rel-L2 {err:.3e}")
    assert err < 1e-2
    attention_elementwise(out, q, k, v, heads, D, f"attention stale-reference d64 Nk={Nk}")


def test_attention_refuses_head_dims_it_does_not_build(sdlib):
    x = torch.zeros(1, 16, 96, dtype=torch.bfloat16, device="cuda")
    assert sdlib.sd_op_attention(stream(), P(x), 96, P(x), 96, P(x), 96, P(torch.zeros_like(x)), 96, 1, 2, 16, 16, 48, 0.1) != 0
    assert b"head dim 48 not supported (40, 64, 80, 160)" in sdlib.sd_last_error()


# ------------------------------------------------------------------------------------------------ the SD 2 UNet at 16x16
@pytest.fixture(scope="module")
def sd2():
    from sonicdiffusionbayeslab_amd.unet import HipUNet2DConditionModel
    from sonicdiffusionbayeslab_amd.weights import make_synthetic_state_dict, sd2_unet_config
    from tests.sd2_oracle import oracle_config
    cfg = sd2_unet_config(16)
    sd = make_synthetic_state_dict(cfg, seed=1234)
    assert sd["mid_block.attentions.0.proj_in.weight"].dim() == 2
    os.environ["SD_DEBUG_TAPS"] = "1"
    try:
        net = HipUNet2DConditionModel(cfg, sd)
    finally:
        os.environ.pop("SD_DEBUG_TAPS")
    return cfg, sd, net, oracle_config(cfg)


@pytest.mark.parametrize("t", [981.0, 21.0])
def test_sd2_unet_forward_matches_oracle(sd2, t):
    from tests.sd2_oracle import sd2_unet_forward
    cfg, sd, net, ocfg = sd2
    lat, pe, ne = synth_inputs(cfg, 1)
    assert pe.shape[-1] == 1024
    ctx = torch.cat([ne, pe])
    taps = {}
    ref = sd2_unet_forward(sd, ocfg, cfg.heads_per_level, torch.cat([lat, lat]), t, ctx, taps=taps)
    net.set_deepcache(-1)
    net.set_context(ctx.cuda())
    eps = net.forward_latents(lat.cuda(), 2, t)
    torch.cuda.synchronize()
    report = []
    for name, rt in taps.items():
        got = net.debug_tensor(name, 2, rt.numel()).view(rt.shape[0], rt.shape[2], rt.shape[3], rt.shape[1])
        report.append((name, round(rel_l2(got.permute(0, 3, 1, 2), rt), 5)))
    err = rel_l2(eps, ref)
    print(f"SD 2 UNet t={t}: per block {report} final {err:.3e} cos {cosine(eps, ref):.5f}")
    assert torch.isfinite(eps).all()
    assert err < UNET_TOL, report


def test_folded_prompt_attention_at_twenty_heads_matches_oracle():
    """At 16x16 latents no level of the SD 2 UNet meets the folded two-GEMM form's conditions (256 tokens at the 5-head level:
    5 x 80 key slots are no multiple of 64; 64 / 16 / 4 tokens below it).  In a 512-pixel image the 20-head level has 256
    tokens and takes it: here a two-level UNet puts 20 heads of 64 on 256 tokens (1600 key slots), with the mid block on
    `to_q` + 77-key attention + `to_out`.  The launch count says which form ran."""
    from sonicdiffusionbayeslab_amd.unet import HipUNet2DConditionModel
    from sonicdiffusionbayeslab_amd.weights import UNetConfig, make_synthetic_state_dict
    from tests.sd2_oracle import oracle_config, sd2_unet_forward
    cfg = UNetConfig(sample_size=16, block_out_channels=(1280, 1280), attn_levels=(True, False), cross_attention_dim=1024,
                     num_heads=20, num_heads_per_level=(20, 20), use_linear_projection=True)
    sd = make_synthetic_state_dict(cfg, seed=77)
    net = HipUNet2DConditionModel(cfg, sd)
    lat, pe, ne = synth_inputs(cfg, 1, seed=71)
    ctx, t = torch.cat([ne, pe]), 501.0
    ref = sd2_unet_forward(sd, oracle_config(cfg), cfg.heads_per_level, torch.cat([lat, lat]), t, ctx)
    net.set_context(ctx.cuda())
    eps = net.forward_latents(lat.cuda(), 2, t).clone()
    prof = net.forward_profiled(lat.cuda(), 2, t)
    err = rel_l2(eps, ref)
    print(f"two-level UNet, 20 heads on 256 tokens (folded prompt attention): rel-L2 {err:.3e} cos {cosine(eps, ref):.5f}; "
          f"attention launches {prof['attention']['launches']}")
    assert prof["attention"]["launches"] == 5 + 2        # five self-attentions at the top level; self + prompt attention in the mid block
    assert torch.isfinite(eps).all() and err < UNET_TOL


def test_sd2_deepcache_skip_forward_matches_oracle(sd2):
    from oracle.unet import DeepCacheState
    from sonicdiffusionbayeslab_amd.unet import CACHE_FULL_AND_STORE, CACHE_SKIP
    from tests.sd2_oracle import sd2_unet_forward
    cfg, sd, net, ocfg = sd2
    lat, pe, ne = synth_inputs(cfg, 1, seed=31)
    lat2 = lat + 0.1 * torch.randn(lat.shape, generator=torch.Generator().manual_seed(32))
    ctx = torch.cat([ne, pe])
    dc = DeepCacheState(cache_interval=3, cache_branch_id=0, enabled=True)
    dc.cur_timestep = 0
    ref_full = sd2_unet_forward(sd, ocfg, cfg.heads_per_level, torch.cat([lat, lat]), 981.0, ctx, dc=dc)
    dc.cur_timestep = 1
    ref_skip = sd2_unet_forward(sd, ocfg, cfg.heads_per_level, torch.cat([lat2, lat2]), 961.0, ctx, dc=dc)
    net.set_deepcache(0)
    try:
        net.set_context(ctx.cuda())
        full = net.forward_latents(lat.cuda(), 2, 981.0, cache_mode=CACHE_FULL_AND_STORE).clone()
        skip = net.forward_latents(lat2.cuda(), 2, 961.0, cache_mode=CACHE_SKIP).clone()
        torch.cuda.synchronize()
    finally:
        net.set_deepcache(-1)
    e_full, e_skip = rel_l2(full, ref_full), rel_l2(skip, ref_skip)
    print(f"SD 2 DeepCache branch 0: full+store rel-L2 {e_full:.3e}, skip step {e_skip:.3e}")
    assert torch.isfinite(skip).all() and e_full < UNET_TOL and e_skip < UNET_TOL


def test_sd2_controlnet_step_matches_oracle(sd2):
    from sonicdiffusionbayeslab_amd.controlnet import HipControlNetModel
    from sonicdiffusionbayeslab_amd.weights import controlnet_config_for, make_synthetic_controlnet_state_dict
    from tests.sd2_oracle import sd2_controlnet_forward, sd2_unet_forward
    cfg, sd, net, ocfg = sd2
    cn = controlnet_config_for(cfg)
    cw = make_synthetic_controlnet_state_dict(cn, seed=1234)
    assert cw["mid_block.attentions.0.proj_in.weight"].dim() == 2 and cn.unet.heads_per_level == cfg.heads_per_level
    cnet = HipControlNetModel(cn, cw)
    lat, pe, ne = synth_inputs(cfg, 1, seed=41)
    ctx = torch.cat([ne, pe])
    cond = torch.rand(1, 3, 128, 128, generator=torch.Generator().manual_seed(42))
    x2, t = torch.cat([lat, lat]), 501.0
    down, mid = sd2_controlnet_forward(cw, ocfg, cfg.heads_per_level, x2, t, ctx, cond)
    ref_on = sd2_unet_forward(sd, ocfg, cfg.heads_per_level, x2, t, ctx, down_residuals=down, mid_residual=mid)
    ref_off = sd2_unet_forward(sd, ocfg, cfg.heads_per_level, x2, t, ctx)
    from sonicdiffusionbayeslab_amd.controlnet import unpack_residuals
    cnet.set_context(ctx.cuda(), 16, 16)
    cnet.set_cond(cond)
    buf = cnet.forward_residuals(lat.cuda(), 2, t)
    torch.cuda.synchronize()
    gd, gm = unpack_residuals(buf, cnet.config, 2, 16, 16)
    errs = [rel_l2(a.cpu(), b) for a, b in zip(list(gd) + [gm], down + [mid])]
    net.set_deepcache(-1)
    net.set_context(ctx.cuda())
    net.set_control_residuals(buf, 1.0, 2, 16, 16)
    try:
        on = net.forward_latents(lat.cuda(), 2, t).clone()
        torch.cuda.synchronize()
    finally:
        net.clear_control_residuals()
    e_on = rel_l2(on, ref_on)
    print(f"SD 2 ControlNet step: residuals rel-L2 max {max(errs):.3e}; UNet with residuals {e_on:.3e}; "
          f"with vs without (oracle) {rel_l2(ref_on, ref_off):.3e}")
    assert max(errs) < UNET_TOL and torch.isfinite(on).all() and e_on < UNET_TOL
    assert rel_l2(on, ref_off) > 10 * UNET_TOL          # the residuals moved the output


def test_sd2_fp8_forward_matches_emulating_oracle(sd2):
    from oracle.fp8 import Fp8Emulation
    from sonicdiffusionbayeslab_amd.unet import HipUNet2DConditionModel
    from tests.sd2_oracle import conv_view, sd2_unet_forward
    cfg, sd, _, ocfg = sd2
    net = HipUNet2DConditionModel(cfg, sd, weight_dtype="fp8")
    assert net.weight_dtype == "fp8_e4m3"
    lat, pe, ne = synth_inputs(cfg, 1)
    ctx, t = torch.cat([ne, pe]), 981.0
    x2 = torch.cat([lat, lat])
    ref_q = sd2_unet_forward(sd, ocfg, cfg.heads_per_level, x2, t, ctx, fq=Fp8Emulation(conv_view(sd)))
    ref = sd2_unet_forward(sd, ocfg, cfg.heads_per_level, x2, t, ctx)
    net.set_context(ctx.cuda())
    eps = net.forward_latents(lat.cuda(), 2, t)
    torch.cuda.synchronize()
    e_q = rel_l2(eps, ref_q)
    print(f"SD 2 fp8 forward t={t}: vs emulating oracle {e_q:.3e} (cos {cosine(eps, ref_q):.5f}); vs unquantised oracle "
          f"{rel_l2(eps, ref):.3e}; oracle fp8-vs-fp32 {rel_l2(ref_q, ref):.3e}")
    assert torch.isfinite(eps).all() and e_q < FWD_TOL and cosine(eps, ref) > 0.99


def test_constant_per_level_heads_are_bit_identical_to_num_heads():
    """SD-1.5 at 32x32 latents (the 8-head fused cross-attention runs at the top level, the folded form below): a handle with
    ``num_heads_per_level=(8, 8, 8, 8)`` runs the plans of ``num_heads=8``."""
    from sonicdiffusionbayeslab_amd.unet import HipUNet2DConditionModel
    from sonicdiffusionbayeslab_amd.weights import UNetConfig, make_synthetic_state_dict
    cfg = UNetConfig(sample_size=32)
    sd = make_synthetic_state_dict(cfg, seed=1234)
    a = HipUNet2DConditionModel(cfg, sd)
    b = HipUNet2DConditionModel(dataclasses.replace(cfg, num_heads_per_level=(8, 8, 8, 8)), sd)
    lat, pe, ne = synth_inputs(cfg, 2, seed=13)
    ctx = torch.cat([ne, pe]).cuda()
    outs = []
    for n in (a, b):
        n.set_context(ctx)
        outs.append(n.forward_latents(lat.cuda(), 4, 501.0).clone())
    torch.cuda.synchronize()
    assert torch.isfinite(outs[0]).all() and torch.equal(outs[0], outs[1])
    pa, pb = a.forward_profiled(lat.cuda(), 4, 501.0), b.forward_profiled(lat.cuda(), 4, 501.0)
    assert {k: v["launches"] for k, v in pa.items()} == {k: v["launches"] for k, v in pb.items()}


# ------------------------------------------------------------------------------------------------ text tower
def test_gelu_text_tower_matches_golden_and_oracle(tmp_path):
    from oracle.clip import ClipTextConfig as OC
    from safetensors.torch import save_file
    from sonicdiffusionbayeslab_amd.clip import ClipPromptEncoder, ClipTextConfig, HipClipTextModel
    from tests.sd2_oracle import clip_text_forward_act, gelu_clip_state_dict
    gold = json.load(open(GOLDEN))
    kw, sd = gelu_clip_state_dict()
    ids = torch.tensor(gold["input_ids"])
    want = torch.tensor(gold["last_hidden_state"])
    ref = clip_text_forward_act(sd, OC(**kw), ids, "gelu")
    out = HipClipTextModel(ClipTextConfig(**kw, hidden_act="gelu"), sd).encode(ids)
    quick = HipClipTextModel(ClipTextConfig(**kw), sd).encode(ids)
    e_g, e_o, e_q = rel_l2(out, want), rel_l2(out, ref), rel_l2(quick, want)
    print(f"tiny gelu text tower: vs transformers golden rel-L2 {e_g:.3e}, vs oracle {e_o:.3e}; a quick_gelu handle on the same "
          f"ids is {e_q:.3e} from the golden")
    assert out.dtype == torch.float32 and tuple(out.shape) == (len(CLIP_TEXTS), 16, 64)
    assert e_g < CLIP_TOL and e_o < CLIP_TOL and cosine(out, ref) > 0.9995
    assert e_q > CLIP_TOL
    # a local SD 2.x-shaped directory: from_pretrained reads hidden_act and the tokenizer's pad token
    vocab, merges = synthetic_clip_vocab()
    os.makedirs(tmp_path / "tokenizer"), os.makedirs(tmp_path / "text_encoder")
    (tmp_path / "tokenizer" / "vocab.json").write_text(json.dumps(vocab))
    (tmp_path / "tokenizer" / "merges.txt").write_text("#version: 0.2\n" + "\n".join(f"{a} {b}" for a, b in merges) + "\n")
    (tmp_path / "tokenizer" / "special_tokens_map.json").write_text(json.dumps({"pad_token": "!"}))
    (tmp_path / "tokenizer" / "tokenizer_config.json").write_text(json.dumps({"pad_token": "!", "model_max_length": 16}))
    (tmp_path / "text_encoder" / "config.json").write_text(json.dumps({**kw, "hidden_act": "gelu", "layer_norm_eps": 1e-5,
                                                                      "model_type": "clip_text_model"}))
    save_file({k: v.contiguous() for k, v in sd.items()}, str(tmp_path / "text_encoder" / "model.safetensors"))
    enc = ClipPromptEncoder.from_pretrained(str(tmp_path))
    enc.tokenizer.model_max_length = 16
    assert enc.text_model.config.hidden_act == "gelu" and enc.tokenizer.pad_token_id == vocab["!"] == enc.text_model.config.pad_token_id
    assert enc.tokenizer(CLIP_TEXTS).tolist() == gold["input_ids"]
    assert torch.equal(enc(CLIP_TEXTS), out)


# ------------------------------------------------------------------------------------------------ free-running loops
def _model(sd2):
    from sonicdiffusionbayeslab_amd.models import StableDiffusionModel
    cfg, sd, net, _ = sd2
    model = StableDiffusionModel(unet_config=cfg, state_dict=dict(sd))
    model.unet = net                    # (the module's handle: building another costs a second packing of 865 M parameters)
    net.set_deepcache(-1)
    return model.to("cuda:0")


def test_sd2_ddim_v_prediction_loop_with_rescaled_cfg(sd2):
    from tests.sd2_oracle import cfg_loop
    cfg, sd, net, ocfg = sd2
    model = _model(sd2)
    n = 3
    model.scheduler, ref_s = R.make_pair("ddim", n, "v_prediction")
    lat, pe, ne = synth_inputs(cfg, 2, seed=53)
    out, _, x0s = model(prompt_embeds=pe, negative_prompt_embeds=ne, latents=lat, num_inference_steps=n, guidance_scale=7.5,
                        guidance_rescale=0.7, output_type="latent")
    ts = list(model.scheduler._timesteps_list)
    ref = cfg_loop(sd, ocfg, cfg.heads_per_level, pe, ne, lat, [(ref_s, t) for t in ts], 7.5, 0.7)
    err, cs = rel_l2(out.images, ref), cosine(out.images, ref)
    print(f"SD 2 DDIM v-prediction, CFG 7.5, guidance_rescale 0.7, {n} steps: rel-L2 {err:.3e} cos {cs:.5f}")
    assert len(x0s) == n and model.scheduler.rescale_factors is not None
    assert err < FREE_TOL and cs > FREE_COS


def test_sd2_dpm_solver_loop(sd2):
    from tests.sd2_oracle import cfg_loop
    cfg, sd, net, ocfg = sd2
    model = _model(sd2)
    n = 2
    model.scheduler, ref_s = R.make_pair("dpm", n, "v_prediction", solver_order=2, algorithm_type="dpmsolver++", final_sigmas_type="zero")
    lat, pe, ne = synth_inputs(cfg, 2, seed=59)
    out, _, _ = model(prompt_embeds=pe, negative_prompt_embeds=ne, latents=lat, num_inference_steps=n, guidance_scale=7.5,
                      output_type="latent")
    ts = list(model.scheduler._timesteps_list)
    ref = cfg_loop(sd, ocfg, cfg.heads_per_level, pe, ne, lat, [(ref_s, t) for t in ts], 7.5, 0.0)
    err, cs = rel_l2(out.images, ref), cosine(out.images, ref)
    print(f"SD 2 DPM-Solver++ 2 (v-prediction), CFG 7.5, {n} steps: rel-L2 {err:.3e} cos {cs:.5f}")
    assert err < FREE_TOL and cs > FREE_COS
