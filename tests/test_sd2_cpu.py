"""Stable Diffusion 2.x on the host: config parsing (per-level head counts, Linear projections, upcast_attention), what is
still refused by name, the library's per-level config and packing, the SD 2 oracle (tests/sd2_oracle.py) against the SD-1.5
one and against the transformers golden of the gelu text tower, and the tokenizer's pad token.  No GPU."""
import ctypes as C
import dataclasses
import json
import math
import os

import pytest
import torch

from sonicdiffusionbayeslab_amd import _lib
from sonicdiffusionbayeslab_amd.weights import (SD2_HEADS, UNetConfig, check_controlnet_pairs, controlnet_config_for,
                                                make_synthetic_state_dict, param_shapes, read_controlnet_config,
                                                read_unet_config, sd2_unet_config)
from tests.util import CLIP_TEXTS, CLIP_TINY, rel_l2, synthetic_clip_vocab

# unet/config.json of stabilityai/stable-diffusion-2-1 (the 768-pixel v-prediction checkpoint)
SD21_UNET_CONFIG = {
    "_class_name": "UNet2DConditionModel", "_diffusers_version": "0.10.0.dev0", "act_fn": "silu",
    "attention_head_dim": [5, 10, 20, 20], "block_out_channels": [320, 640, 1280, 1280], "center_input_sample": False,
    "cross_attention_dim": 1024,
    "down_block_types": ["CrossAttnDownBlock2D", "CrossAttnDownBlock2D", "CrossAttnDownBlock2D", "DownBlock2D"],
    "downsample_padding": 1, "dual_cross_attention": False, "flip_sin_to_cos": True, "freq_shift": 0, "in_channels": 4,
    "layers_per_block": 2, "mid_block_scale_factor": 1, "norm_eps": 1e-05, "norm_num_groups": 32, "num_class_embeds": None,
    "only_cross_attention": False, "out_channels": 4, "sample_size": 96,
    "up_block_types": ["UpBlock2D", "CrossAttnUpBlock2D", "CrossAttnUpBlock2D", "CrossAttnUpBlock2D"],
    "upcast_attention": True, "use_linear_projection": True,
}
GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "clip_gelu_golden.json")


def _c_config(cfg, dtype="bf16"):
    from sonicdiffusionbayeslab_amd.unet import _c_config as cc
    return cc(cfg, dtype)


def _create(lib, ccfg):
    h = C.c_void_p()
    return lib.sd_unet_create(C.byref(ccfg), C.byref(h)), h


# ------------------------------------------------------------------------------------------------ config
def test_sd21_unet_config_parses():
    cfg = read_unet_config(SD21_UNET_CONFIG)
    assert cfg.heads_per_level == (5, 10, 20, 20) == SD2_HEADS and cfg.num_heads_per_level == (5, 10, 20, 20)
    assert cfg.cross_attention_dim == 1024 and cfg.sample_size == 96 and cfg.use_linear_projection is True
    assert cfg.block_out_channels == (320, 640, 1280, 1280) and cfg.attn_levels == (True, True, True, False)
    assert cfg == sd2_unet_config(96)
    # the flags survive dataclasses.replace and stay out of asdict (the SD-1.5 oracle's config is built from it)
    small = dataclasses.replace(cfg, sample_size=16)
    assert small.heads_per_level == SD2_HEADS and small.use_linear_projection and "num_heads_per_level" not in dataclasses.asdict(small)
    assert small != dataclasses.replace(small, num_heads_per_level=None) and small != dataclasses.replace(small, use_linear_projection=False)
    shapes = dict(param_shapes(cfg))
    assert shapes["down_blocks.1.attentions.0.proj_in.weight"] == (640, 640)
    assert shapes["mid_block.attentions.0.proj_out.weight"] == (1280, 1280)
    assert shapes["down_blocks.0.attentions.0.transformer_blocks.0.attn2.to_k.weight"] == (320, 1024)
    # -2-inpainting: the same UNet with nine input channels
    inp = read_unet_config({**SD21_UNET_CONFIG, "in_channels": 9, "sample_size": 64})
    assert inp.in_channels == 9 and inp == sd2_unet_config(64, in_channels=9)


def test_head_rule_is_diffusers():
    """``num_attention_heads`` wins where it is present and not null; otherwise ``attention_head_dim`` is the head COUNT."""
    base = {k: v for k, v in SD21_UNET_CONFIG.items() if k != "attention_head_dim"}
    assert read_unet_config({**base, "attention_head_dim": 8, "cross_attention_dim": 768}).heads_per_level == (8, 8, 8, 8)
    assert read_unet_config({**base, "attention_head_dim": [8, 8, 8, 8]}).num_heads_per_level is None      # constant: SD-1.5's form
    assert read_unet_config({**base, "attention_head_dim": 8, "num_attention_heads": [5, 10, 20, 20]}).heads_per_level == SD2_HEADS
    assert read_unet_config({**base, "attention_head_dim": [5, 10, 20, 20], "num_attention_heads": None}).heads_per_level == SD2_HEADS
    assert read_unet_config({**base, "attention_head_dim": [5, 10, 20, 20], "num_attention_heads": 8}).heads_per_level == (8, 8, 8, 8)
    for bad in ([5, 10, 20], [5, 10, 0, 20], "8", 0, True):
        with pytest.raises(NotImplementedError, match="attention_head_dim"):
            read_unet_config({**base, "attention_head_dim": bad})
    with pytest.raises(ValueError, match="num_heads_per_level"):
        UNetConfig(num_heads_per_level=(5, 10, 20))


@pytest.mark.parametrize("key,value", [
    ("dual_cross_attention", True), ("only_cross_attention", True), ("class_embed_type", "timestep"), ("num_class_embeds", 1000),
    ("addition_embed_type", "text_time"), ("in_channels", 5), ("in_channels", 8), ("transformer_layers_per_block", 2),
    ("transformer_layers_per_block", [1, 2, 10]), ("use_linear_projection", "yes"), ("upcast_attention", 1),
    ("act_fn", "gelu"), ("down_block_types", ["CrossAttnDownBlock2D", "SimpleCrossAttnDownBlock2D", "CrossAttnDownBlock2D", "DownBlock2D"]),
])
def test_keys_still_refused_by_name(key, value):
    with pytest.raises(NotImplementedError, match=key):
        read_unet_config({**SD21_UNET_CONFIG, key: value})


def test_controlnet_pairs_on_the_per_level_heads():
    cfg = sd2_unet_config(16)
    cn = controlnet_config_for(cfg)
    assert cn.unet.heads_per_level == SD2_HEADS and cn.unet.use_linear_projection
    check_controlnet_pairs(cn, cfg)
    with pytest.raises(ValueError, match="heads_per_level"):
        check_controlnet_pairs(cn, UNetConfig(sample_size=16, cross_attention_dim=1024))
    # an SD-1.5 pair: None and the constant tuple are the same heads
    check_controlnet_pairs(controlnet_config_for(UNetConfig()), UNetConfig(num_heads_per_level=(8, 8, 8, 8)))
    got = read_controlnet_config({k: v for k, v in SD21_UNET_CONFIG.items() if k != "up_block_types"}, cfg)
    assert got.unet.heads_per_level == SD2_HEADS


def test_from_pretrained_shapes_the_stand_in_and_refuses_conflicts(tmp_path):
    from safetensors.torch import save_file
    from sonicdiffusionbayeslab_amd.models import StableDiffusionModel
    m = StableDiffusionModel.from_pretrained("stabilityai/stable-diffusion-2-1", unet_arch="sd2", sample_size=96,
                                             prediction_type="v_prediction")
    assert m.unet_config == sd2_unet_config(96) and m.scheduler.config.prediction_type == "v_prediction"
    assert m.weights_source.startswith("synthetic(") and m.text_encoder.dim == 1024
    assert StableDiffusionModel.from_pretrained("runwayml/stable-diffusion-v1-5").unet_config == UNetConfig()
    with pytest.raises(ValueError, match="unet_arch"):
        StableDiffusionModel.from_pretrained("x/y", unet_arch="sdxl")
    # a local SD 2.x-shaped directory: its own files decide; a conflicting key is an error
    cfg = UNetConfig(sample_size=8, block_out_channels=(320, 640), attn_levels=(True, False), cross_attention_dim=1024,
                     num_heads=5, num_heads_per_level=(5, 10), use_linear_projection=True)
    sd = make_synthetic_state_dict(cfg, seed=3)
    os.makedirs(tmp_path / "unet"), os.makedirs(tmp_path / "scheduler")
    cj = {**SD21_UNET_CONFIG, "sample_size": 8, "block_out_channels": [320, 640], "attention_head_dim": [5, 10],
          "down_block_types": ["CrossAttnDownBlock2D", "DownBlock2D"], "up_block_types": ["UpBlock2D", "CrossAttnUpBlock2D"]}
    (tmp_path / "unet" / "config.json").write_text(json.dumps(cj))
    (tmp_path / "scheduler" / "scheduler_config.json").write_text(json.dumps({"_class_name": "DDIMScheduler", "prediction_type": "v_prediction"}))
    save_file({k: v.half() for k, v in sd.items()}, str(tmp_path / "unet" / "diffusion_pytorch_model.safetensors"))
    m = StableDiffusionModel.from_pretrained(str(tmp_path), prediction_type="v_prediction", sample_size=8)
    assert m.unet_config == cfg and m.scheduler.config.prediction_type == "v_prediction"
    assert tuple(m._state_dict["down_blocks.0.attentions.0.proj_in.weight"].shape) == (320, 320)
    for kw, what in ((dict(unet_arch="sd2"), "unet_arch"), (dict(sample_size=96), "sample_size"), (dict(prediction_type="epsilon"), "prediction_type")):
        with pytest.raises(ValueError, match=what):      # (two levels of (5, 10) heads are not the SD 2.x family's four)
            StableDiffusionModel.from_pretrained(str(tmp_path), **kw)
    # config and weights must agree on the projection layout
    (tmp_path / "unet" / "config.json").write_text(json.dumps({**cj, "use_linear_projection": False}))
    with pytest.raises(NotImplementedError, match="use_linear_projection"):
        StableDiffusionModel.from_pretrained(str(tmp_path))


# ------------------------------------------------------------------------------------------------ library
def test_library_takes_the_per_level_config_and_the_abi_stays():
    lib = _lib.load()
    assert lib.sd_abi_version() == 3
    assert [f[0] for f in _lib.SdUnetConfigFull._fields_] == ["num_heads_per_level"]         # appended behind the ABI-3 fields
    assert C.sizeof(_lib.SdUnetConfigFull) == C.sizeof(_lib.SdUnetConfig) + 8 * 4
    assert _lib.SdUnetConfigFull.num_heads_per_level.offset == C.sizeof(_lib.SdUnetConfig)
    cfg = sd2_unet_config(16)
    c = _c_config(cfg)
    assert list(c.num_heads_per_level) == [5, 10, 20, 20, 0, 0, 0, 0] and list(_c_config(UNetConfig()).num_heads_per_level) == [0] * 8
    rc, h = _create(lib, c)
    assert rc == 0, lib.sd_last_error()
    # the parameter table keeps the 1x1-conv shape of proj_in / proj_out: the host normalises a Linear weight
    name, shape, nd = C.create_string_buffer(256), (C.c_longlong * 4)(), C.c_int()
    got = {}
    for i in range(lib.sd_unet_num_params(h)):
        _lib.check(lib.sd_unet_param_info(h, i, name, 256, shape, C.byref(nd)))
        got[name.value.decode()] = tuple(shape[k] for k in range(nd.value))
    lib.sd_unet_destroy(h)
    want = dict(param_shapes(cfg))
    assert set(got) == set(want)
    assert all(got[n] == (s + (1, 1) if n.endswith(("proj_in.weight", "proj_out.weight")) else s) for n, s in want.items())
    # all zeros and the constant tuple are SD-1.5; a partial list and a level past num_levels are refused by name
    for heads in ((8, 8, 8, 8),):
        rc, h = _create(lib, _c_config(UNetConfig(sample_size=16, num_heads_per_level=heads)))
        assert rc == 0, lib.sd_last_error()
        lib.sd_unet_destroy(h)
    c = _c_config(cfg); c.num_heads_per_level[2] = 0
    rc, _ = _create(lib, c)
    assert rc != 0 and b"num_heads_per_level names 3 of 4 levels" in lib.sd_last_error()
    c = _c_config(cfg); c.num_heads_per_level[5] = 4
    rc, _ = _create(lib, c)
    assert rc != 0 and b"num_heads_per_level[5]=4" in lib.sd_last_error()


def test_library_refuses_head_dims_it_does_not_build_by_name():
    lib = _lib.load()
    rc, _ = _create(lib, _c_config(UNetConfig(sample_size=16, block_out_channels=(384, 768, 1536, 1536))))      # 8 heads of 48 / 96 / 192
    assert rc != 0 and b"head dim 48 at level 0 (384 channels, 8 heads) not built (40/64/80/160)" in lib.sd_last_error()
    rc, _ = _create(lib, _c_config(UNetConfig(sample_size=16, num_heads_per_level=(5, 10, 20, 40))))            # mid block: 1280 / 40 = 32
    assert rc != 0 and b"mid-block head dim 32 (1280 channels, 40 heads)" in lib.sd_last_error()
    rc, _ = _create(lib, _c_config(UNetConfig(sample_size=16, num_heads_per_level=(5, 10, 7, 20))))
    assert rc != 0 and b"at level 2 (1280 channels, 7 heads)" in lib.sd_last_error()
    # an IP-Adapter stays refused on head counts ip_xattn does not build; the message names the level's count
    rc, _ = _create(lib, _c_config(dataclasses.replace(sd2_unet_config(16), ip_adapter_embed_dim=128)))
    assert rc != 0 and b"an IP-Adapter needs 1, 2, 4 or 8 heads" in lib.sd_last_error() and b"(level 0: 320 channels, 5 heads)" in lib.sd_last_error()
    # text tower: hidden_act is 0 (quick_gelu) or 1 (gelu)
    h = C.c_void_p()
    assert lib.sd_clip_create(C.byref(_lib.SdClipConfig(100, 64, 1, 4, 128, 16, 1e-5, 2)), C.byref(h)) != 0
    assert b"hidden_act 2" in lib.sd_last_error()
    for act in (0, 1):
        _lib.check(lib.sd_clip_create(C.byref(_lib.SdClipConfig(100, 64, 1, 4, 128, 16, 1e-5, act)), C.byref(h)))
        lib.sd_unet_destroy(h)


def _sd2_like_handles(lib):
    from sonicdiffusionbayeslab_amd.unet import load_params
    kw = dict(sample_size=8, block_out_channels=(320, 640), attn_levels=(True, True), cross_attention_dim=64, num_heads=5,
              num_heads_per_level=(5, 10))
    lin, conv = UNetConfig(**kw, use_linear_projection=True), UNetConfig(**kw)
    sd_lin, sd_conv = make_synthetic_state_dict(lin, seed=5), make_synthetic_state_dict(conv, seed=5)
    handles = []
    for cfg, sd in ((lin, sd_lin), (conv, sd_conv)):
        rc, h = _create(lib, _c_config(cfg))
        assert rc == 0, lib.sd_last_error()
        load_params(lib, h, cfg, sd)
        handles.append(h)
    return lin, sd_lin, sd_conv, handles


def test_load_params_checks_the_projection_layout_of_the_config():
    from sonicdiffusionbayeslab_amd.unet import load_params
    lib = _lib.load()
    lin, sd_lin, sd_conv, handles = _sd2_like_handles(lib)
    pin = "down_blocks.1.attentions.0.proj_in.weight"
    assert sd_lin[pin].shape == (640, 640) and torch.equal(sd_lin[pin][:, :, None, None], sd_conv[pin])
    with pytest.raises(ValueError, match="proj_in.weight"):          # the shape is checked against the CONFIG's layout
        load_params(lib, handles[0], lin, sd_conv)
    for h in handles:
        lib.sd_unet_destroy(h)


def test_packing_per_level_scale_and_linear_projection():
    """``attn1`` W_q carries log2(e) / sqrt(d) of ITS level (10 heads at 640 channels: d = 64), and a [C, C] ``proj_in`` packs
    to the bytes of the same weight given as [C, C, 1, 1].  The packer runs on the host BEFORE the upload and the staging blob
    is released after a successful one, so the packed bytes can be read only where there is no device (as
    tests/test_host_cpu.py::test_finalize_packs_weights_on_the_host)."""
    if torch.cuda.is_available():
        pytest.skip("host-side packer check runs on the CPU-only box (the blob is released after a successful upload)")
    lib = _lib.load()
    lin, sd_lin, sd_conv, handles = _sd2_like_handles(lib)
    pin = "down_blocks.1.attentions.0.proj_in.weight"

    def packed(h, key, n):
        buf = torch.empty(n, dtype=torch.bfloat16)
        assert lib.sd_unet_debug_packed(h, key.encode(), buf.data_ptr(), n * 2) >= 0, lib.sd_last_error()
        return buf
    for h in handles:
        assert lib.sd_unet_finalize(h) == -2 and b"hipMalloc" in lib.sd_last_error()
    for key, n in ((pin, 640 * 640), ("down_blocks.0.attentions.1.proj_out.weight", 320 * 320), ("mid_block.attentions.0.ff_out.weight", 640 * 3200)):
        a, b = packed(handles[0], key, n), packed(handles[1], key, n)
        assert torch.equal(a.view(torch.int16), b.view(torch.int16)), key
    assert torch.equal(packed(handles[0], pin, 640 * 640).float().view(640, 640), sd_lin[pin])
    for blk, c, heads in (("down_blocks.0.attentions.0.", 320, 5), ("down_blocks.1.attentions.1.", 640, 10),
                          ("mid_block.attentions.0.", 640, 10), ("up_blocks.0.attentions.2.", 640, 10), ("up_blocks.1.attentions.0.", 320, 5)):
        t = blk + "transformer_blocks.0."
        qkv = packed(handles[0], t + "attn1.qkv.weight", 3 * c * c).float().view(3 * c, c)
        assert c // heads == 64
        qs = torch.tensor(1.4426950408889634, dtype=torch.float32) / math.sqrt(64.0)
        assert torch.equal(qkv[:c], (sd_lin[t + "attn1.to_q.weight"] * qs).bfloat16().float()), blk
        assert torch.equal(qkv[c:2 * c], sd_lin[t + "attn1.to_k.weight"]) and torch.equal(qkv[2 * c:], sd_lin[t + "attn1.to_v.weight"])
    for h in handles:
        lib.sd_unet_destroy(h)


# ------------------------------------------------------------------------------------------------ oracle
TINY = dict(sample_size=8, block_out_channels=(64, 128, 128, 128), num_heads=2, cross_attention_dim=64, context_len=5)


def test_sd2_oracle_equals_the_sd15_oracle_on_constant_heads():
    from oracle.unet import DeepCacheState, unet_forward
    from tests.sd2_oracle import conv_view, oracle_config, sd2_unet_forward
    cfg = UNetConfig(**TINY)
    sd = make_synthetic_state_dict(cfg, seed=7)
    g = torch.Generator().manual_seed(1)
    x, ctx = torch.randn(2, 4, 8, 8, generator=g), torch.randn(2, 5, 64, generator=g)
    ocfg = oracle_config(cfg)
    with torch.no_grad():
        ref = unet_forward(sd, ocfg, x, 501, ctx)
    assert torch.equal(sd2_unet_forward(sd, ocfg, (2, 2, 2, 2), x, 501, ctx), ref)
    # Linear projections are the same weights seen as 1x1 convs: the same bits
    lin = make_synthetic_state_dict(dataclasses.replace(cfg, use_linear_projection=True), seed=7)
    assert lin["mid_block.attentions.0.proj_in.weight"].dim() == 2
    assert all(torch.equal(v, sd[k]) for k, v in conv_view(lin).items())
    assert torch.equal(sd2_unet_forward(lin, ocfg, (2, 2, 2, 2), x, 501, ctx), ref)
    # DeepCache: a full step that stores, then a skip step, as the SD-1.5 oracle does them
    outs = []
    for fwd in (lambda dc, t: unet_forward(sd, ocfg, x, t, ctx, dc=dc), lambda dc, t: sd2_unet_forward(lin, ocfg, (2, 2, 2, 2), x, t, ctx, dc=dc)):
        dc = DeepCacheState(cache_interval=2, cache_branch_id=0, enabled=True)
        with torch.no_grad():
            dc.cur_timestep = 0
            a = fwd(dc, 501)
            dc.cur_timestep = 1
            outs.append((a, fwd(dc, 481)))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    # the head count matters, level by level
    for heads in ((4, 2, 2, 2), (2, 2, 4, 2), (2, 2, 2, 4)):
        assert rel_l2(sd2_unet_forward(sd, ocfg, heads, x, 501, ctx), ref) > 1e-3, heads


def test_gelu_text_oracle_matches_the_transformers_golden():
    from oracle.clip import ClipTextConfig as OC, clip_text_forward
    from tests.sd2_oracle import clip_text_forward_act, gelu_clip_state_dict
    gold = json.load(open(GOLDEN))
    kw, sd = gelu_clip_state_dict()
    ids = torch.tensor(gold["input_ids"])
    want = torch.tensor(gold["last_hidden_state"])
    got = clip_text_forward_act(sd, OC(**kw), ids, "gelu")
    assert rel_l2(got, want) < 1e-5
    quick = clip_text_forward_act(sd, OC(**kw), ids, "quick_gelu")
    assert torch.equal(quick, clip_text_forward(sd, OC(**kw), ids))         # the SD-1.5 oracle's tower
    assert rel_l2(quick, want) > 4 * 1.5e-2                                   # the fixture tells the activations apart


def test_tokenizer_pads_with_the_configured_token(tmp_path):
    from sonicdiffusionbayeslab_amd.clip import ClipBpeTokenizer, ClipTextConfig, read_special_tokens
    gold = json.load(open(GOLDEN))
    vocab, merges = synthetic_clip_vocab()
    (tmp_path / "vocab.json").write_text(json.dumps(vocab))
    (tmp_path / "merges.txt").write_text("#version: 0.2\n" + "\n".join(f"{a} {b}" for a, b in merges) + "\n")
    plain = ClipBpeTokenizer.from_pretrained(str(tmp_path))
    assert plain.pad_token_id == vocab["<|endoftext|>"]                       # no file names a pad token: SD-1.5's
    # SD 2.x: special_tokens_map.json says "!" (a string, or a dict with content); it wins over tokenizer_config.json
    (tmp_path / "tokenizer_config.json").write_text(json.dumps({"pad_token": "<|endoftext|>", "model_max_length": 77}))
    (tmp_path / "special_tokens_map.json").write_text(json.dumps({
        "bos_token": {"content": "<|startoftext|>", "lstrip": False, "normalized": True, "rstrip": False, "single_word": False},
        "eos_token": {"content": "<|endoftext|>", "lstrip": False, "normalized": True, "rstrip": False, "single_word": False},
        "pad_token": "!", "unk_token": {"content": "<|endoftext|>"}}))
    assert read_special_tokens(str(tmp_path))["pad_token"] == "!"
    L = CLIP_TINY["max_position_embeddings"]
    tk = ClipBpeTokenizer.from_pretrained(str(tmp_path), model_max_length=L)
    assert tk.pad_token_id == vocab["!"] == 33 and tk.eos_token_id == vocab["<|endoftext|>"]
    assert gold["texts"] == CLIP_TEXTS and gold["pad_token"] == "!"
    assert tk(CLIP_TEXTS).tolist() == gold["input_ids"]
    (tmp_path / "special_tokens_map.json").write_text(json.dumps({"pad_token": {"content": "!"}}))
    assert ClipBpeTokenizer.from_pretrained(str(tmp_path), model_max_length=L)(CLIP_TEXTS).tolist() == gold["input_ids"]
    (tmp_path / "special_tokens_map.json").write_text(json.dumps({"pad_token": "<no such token>"}))
    with pytest.raises(KeyError, match="pad_token"):
        ClipBpeTokenizer.from_pretrained(str(tmp_path))
    (tmp_path / "special_tokens_map.json").write_text(json.dumps({"pad_token": 5}))
    with pytest.raises(ValueError, match="pad_token"):
        ClipBpeTokenizer.from_pretrained(str(tmp_path))
    # the text tower's activation: two are built, anything else is refused by name
    assert ClipTextConfig(hidden_act="gelu").hidden_act == "gelu" and ClipTextConfig().hidden_act == "quick_gelu"
    with pytest.raises(NotImplementedError, match="hidden_act='gelu_new'"):
        ClipTextConfig(hidden_act="gelu_new")
