"""IP-Adapter image prompts without a GPU: the new exports and config fields, the handle's parameter table with and without
an adapter, the checkpoint loader (both container forms, the attn_processors ordering, named errors), known-answer tests of
the oracle (tests/ip_adapter_oracle.py), every argument check before any GPU work, and the harness's shard slicing."""
import ctypes as C
import dataclasses

import pytest
import torch
import torch.nn.functional as F

from sonicdiffusionbayeslab_amd import _lib
from sonicdiffusionbayeslab_amd.weights import IP_ADAPTER_TOKENS, IP_PROJ, UNetConfig, attn2_prefixes, ip_adapter_param_shapes, \
    load_ip_adapter_state_dict, make_synthetic_ip_adapter_state_dict, make_synthetic_state_dict, map_ip_adapter_state_dict, \
    param_shapes, to_upstream_ip_adapter
from tests.ip_xattn_case import EPS, SHAPES as IP_XATTN_SHAPES, operands, perturbed, ref_bound

NEW_SYMBOLS = ["sd_unet_set_ip_adapter_hw", "sd_op_ip_xattn"]
TINY = dict(sample_size=8, block_out_channels=(64, 128, 128, 128), num_heads=2, cross_attention_dim=64, context_len=5)
LIB_SMALL = dict(sample_size=8, block_out_channels=(320, 640), attn_levels=(True, False))      # two levels the library builds
E = 128


def test_symbols_are_exported_and_the_abi_version_stays():
    lib = _lib.load()
    for n in NEW_SYMBOLS:
        assert hasattr(lib, n), n
        assert n in _lib._SIGS and n in _lib.declared_symbols(), n
    assert lib.sd_abi_version() == 3
    names = [f[0] for f in _lib.SdUnetConfig._fields_]
    assert names[-3:] == ["time_cond_proj_dim", "ip_adapter_tokens", "ip_adapter_embed_dim"]       # appended, in this order
    assert len(_lib._SIGS["sd_unet_set_context_hw"][1]) == 9 and len(_lib._SIGS["sd_op_xattn_fused"][1]) == 11


def _enumerate(lib, ccfg):
    h = C.c_void_p()
    _lib.check(lib.sd_unet_create(C.byref(ccfg), C.byref(h)))
    try:
        name, shape, nd = C.create_string_buffer(256), (C.c_longlong * 4)(), C.c_int()
        got = []
        for i in range(lib.sd_unet_num_params(h)):
            _lib.check(lib.sd_unet_param_info(h, i, name, 256, shape, C.byref(nd)))
            got.append((name.value.decode(), tuple(shape[k] for k in range(nd.value))))
        return got
    finally:
        lib.sd_unet_destroy(h)


def test_handle_parameter_table_with_and_without_the_adapter_fields():
    from sonicdiffusionbayeslab_amd.unet import _c_config
    lib = _lib.load()
    for base in (UNetConfig(sample_size=16), UNetConfig(**LIB_SMALL)):
        plain = _enumerate(lib, _c_config(base))
        assert plain == param_shapes(base)                      # zero-initialised fields: names, shapes and count of today
        cfg = dataclasses.replace(base, ip_adapter_embed_dim=E)
        assert cfg.ip_adapter_tokens == IP_ADAPTER_TOKENS
        got = _enumerate(lib, _c_config(cfg))
        assert got == param_shapes(cfg)
        extra = [x for x in got if x not in plain]
        assert extra == ip_adapter_param_shapes(cfg) and [x for x in got if x in plain] == plain
        cd, nblk = base.cross_attention_dim, len(attn2_prefixes(base))
        assert len(extra) == 2 * nblk + 4
        d = dict(extra)
        assert d[IP_PROJ + "image_embeds.weight"] == (4 * cd, E) and d[IP_PROJ + "image_embeds.bias"] == (4 * cd,)
        assert d[IP_PROJ + "norm.weight"] == (cd,) and d[IP_PROJ + "norm.bias"] == (cd,)
        chan = {n[: -len("to_q.weight")]: s[0] for n, s in plain if n.endswith("attn2.to_q.weight")}
        for p in attn2_prefixes(base):
            assert d[p + "processor.to_k_ip.0.weight"] == (chan[p], cd) and d[p + "processor.to_v_ip.0.weight"] == (chan[p], cd)


def test_library_refuses_adapters_it_does_not_build_by_name():
    from sonicdiffusionbayeslab_amd.unet import _c_config
    lib = _lib.load()
    for tokens, e, want in ((16, 1024, b"ip_adapter_tokens 16"), (257, 1280, b"ip_adapter_tokens 257"), (4, 0, b"ip_adapter_embed_dim"),
                            (4, 100, b"ip_adapter_embed_dim"), (0, 1024, b"ip_adapter_tokens 0")):
        c = _c_config(UNetConfig(sample_size=16))
        c.ip_adapter_tokens, c.ip_adapter_embed_dim = tokens, e
        h = C.c_void_p()
        assert lib.sd_unet_create(C.byref(c), C.byref(h)) != 0
        assert want in lib.sd_last_error(), lib.sd_last_error()
    c = _c_config(UNetConfig(sample_size=16, num_heads=5, block_out_channels=(320, 640, 1280, 1280), ip_adapter_embed_dim=E))
    h = C.c_void_p()
    assert lib.sd_unet_create(C.byref(c), C.byref(h)) != 0          # (head dim 64 is refused first; 5 heads are not built either way)
    # a handle without an adapter refuses the entry point by name, before touching the device
    h = C.c_void_p()
    _lib.check(lib.sd_unet_create(C.byref(_c_config(UNetConfig(sample_size=16))), C.byref(h)))
    try:
        assert lib.sd_unet_set_ip_adapter_hw(h, None, 256, 2, -1, 16, 16, 1.0, 256, 1 << 20) != 0
        assert b"without an IP-Adapter" in lib.sd_last_error()
    finally:
        lib.sd_unet_destroy(h)
    # the operator entry point checks its shapes on the host (no device is touched: every call fails in SD_REQUIRE)
    p = 256
    for args, want in (((1.0e-5, 64, 48, 32, 8, 4), b"C=48"), ((1.0e-5, 64, 320, 32, 8, 16), b"T=16"), ((1.0e-5, 64, 320, 32, 3, 4), b"heads=3"),
                       ((1.0e-5, 64, 320, 0, 8, 4), b"rows_per_sample=0"), ((1.0e-5, 65, 320, 32, 8, 4), b"M=65")):
        assert lib.sd_op_ip_xattn(None, p, 512, p, p, p, p, *args) != 0
        assert want in lib.sd_last_error(), lib.sd_last_error()
    assert lib.sd_op_ip_xattn(None, p, p, p, p, p, p, 1.0e-5, 64, 320, 32, 8, 4) != 0 and b"alias" in lib.sd_last_error()


def test_config_fields():
    cfg = UNetConfig(sample_size=16, ip_adapter_embed_dim=1024)
    assert dataclasses.replace(cfg, sample_size=32).ip_adapter_embed_dim == 1024
    assert "ip_adapter_embed_dim" not in dataclasses.asdict(cfg)             # the oracle's config still builds from asdict
    assert cfg != UNetConfig(sample_size=16) and cfg == UNetConfig(sample_size=16, ip_adapter_embed_dim=1024)
    assert UNetConfig().ip_adapter_embed_dim is None and UNetConfig().ip_adapter_tokens is None
    for bad in (0, -64, 100, True):
        with pytest.raises(ValueError, match="ip_adapter_embed_dim"):
            UNetConfig(ip_adapter_embed_dim=bad)
    for t in (16, 257, 1):
        with pytest.raises(NotImplementedError, match="image tokens"):
            UNetConfig(ip_adapter_embed_dim=1024, ip_adapter_tokens=t)
    # the plain parameters of the synthetic generator do not move when an adapter is added
    base = UNetConfig(**TINY)
    a, b = make_synthetic_state_dict(base, 5), make_synthetic_state_dict(dataclasses.replace(base, ip_adapter_embed_dim=E), 5)
    assert a.keys() == b.keys() and all(torch.equal(a[k], b[k]) for k in a)


def test_attn_processor_ordering_is_down_up_mid():
    pre = attn2_prefixes(UNetConfig())
    assert len(pre) == 16
    assert pre[0] == "down_blocks.0.attentions.0.transformer_blocks.0.attn2." and pre[5] == "down_blocks.2.attentions.1.transformer_blocks.0.attn2."
    assert pre[6] == "up_blocks.1.attentions.0.transformer_blocks.0.attn2." and pre[14] == "up_blocks.3.attentions.2.transformer_blocks.0.attn2."
    assert pre[15] == "mid_block.attentions.0.transformer_blocks.0.attn2."


@pytest.mark.parametrize("form", ["bin", "safetensors"])
def test_loader_maps_the_upstream_layout(tmp_path, form):
    base = UNetConfig(**TINY)
    cfg = dataclasses.replace(base, ip_adapter_embed_dim=E)
    sd = make_synthetic_ip_adapter_state_dict(cfg, seed=3)
    up = to_upstream_ip_adapter(sd, cfg)
    n = len(attn2_prefixes(cfg))
    assert sorted(up["ip_adapter"]) == sorted(f"{k}.{w}.weight" for k in range(1, 2 * n, 2) for w in ("to_k_ip", "to_v_ip"))
    assert sorted(up["image_proj"]) == ["norm.bias", "norm.weight", "proj.bias", "proj.weight"]
    if form == "bin":
        path = str(tmp_path / "ip-adapter_sd15.bin")
        torch.save(up, path)
    else:
        from safetensors.torch import save_file
        path = str(tmp_path / "ip-adapter_sd15.safetensors")
        save_file({f"{g}.{k}": v.contiguous() for g, d in up.items() for k, v in d.items()}, path)
    got, e = load_ip_adapter_state_dict(path, base)
    assert e == E and got.keys() == sd.keys() and all(torch.equal(got[k], sd[k]) for k in sd)
    # k = 1, 3, ... in the order down, up, mid: key 2 n - 1 is the MID block's, not the last block of the forward order
    assert torch.equal(got["mid_block.attentions.0.transformer_blocks.0.attn2.processor.to_k_ip.0.weight"],
                       up["ip_adapter"][f"{2 * n - 1}.to_k_ip.weight"])
    assert torch.equal(got["down_blocks.0.attentions.0.transformer_blocks.0.attn2.processor.to_v_ip.0.weight"], up["ip_adapter"]["1.to_v_ip.weight"])
    assert torch.equal(got["up_blocks.1.attentions.0.transformer_blocks.0.attn2.processor.to_k_ip.0.weight"],
                       up["ip_adapter"][f"{2 * len([p for p in attn2_prefixes(cfg) if p.startswith('down')]) + 1}.to_k_ip.weight"])


def test_loader_errors_name_the_key():
    base = UNetConfig(**TINY)
    cfg = dataclasses.replace(base, ip_adapter_embed_dim=E)
    good = to_upstream_ip_adapter(make_synthetic_ip_adapter_state_dict(cfg, seed=3), cfg)
    clone = lambda: {g: dict(d) for g, d in good.items()}
    bad = clone(); del bad["ip_adapter"]["3.to_v_ip.weight"]
    with pytest.raises(KeyError, match=r"ip_adapter\.3\.to_v_ip\.weight"):
        map_ip_adapter_state_dict(bad, base)
    bad = clone(); del bad["image_proj"]["norm.bias"]
    with pytest.raises(KeyError, match=r"image_proj\.norm\.bias"):
        map_ip_adapter_state_dict(bad, base)
    bad = clone(); del bad["image_proj"]
    with pytest.raises(KeyError, match="image_proj"):
        map_ip_adapter_state_dict(bad, base)
    bad = clone(); bad["ip_adapter"]["1.to_k_ip.weight"] = torch.zeros(128, 64)
    with pytest.raises(ValueError, match=r"ip_adapter\.1\.to_k_ip\.weight"):
        map_ip_adapter_state_dict(bad, base)
    bad = clone(); bad["image_proj"]["proj.bias"] = torch.zeros(7)
    with pytest.raises(ValueError, match=r"image_proj\.proj\.bias"):
        map_ip_adapter_state_dict(bad, base)
    bad = clone(); bad["image_proj"]["proj.weight"] = torch.zeros(16 * 64, E)       # 16 tokens: a "plus" projection's count
    with pytest.raises(NotImplementedError, match="16 image tokens"):
        map_ip_adapter_state_dict(bad, base)
    bad = clone(); bad["image_proj"] = {"latents": torch.zeros(1, 16, 64), "proj_in.weight": torch.zeros(64, E)}
    with pytest.raises(NotImplementedError, match="Resampler"):
        map_ip_adapter_state_dict(bad, base)
    with pytest.raises(FileNotFoundError):
        load_ip_adapter_state_dict("/nonexistent/ip-adapter_sd15.bin", base)


# ---------------------------------------------------------------------------------------------------------------------
# the oracle
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny():
    from tests.util import oracle_cfg, synth_inputs
    cfg = UNetConfig(**TINY, ip_adapter_embed_dim=E)
    sd = {**make_synthetic_state_dict(cfg, seed=11), **make_synthetic_ip_adapter_state_dict(cfg, seed=11)}
    lat, pe, ne = synth_inputs(cfg, 2)
    emb = torch.randn(2, E, generator=torch.Generator().manual_seed(4))
    return cfg, oracle_cfg(cfg), sd, lat, pe, ne, emb


def test_oracle_scale_zero_is_the_plain_oracle_exactly(tiny):
    from oracle.unet import unet_forward
    from tests.ip_adapter_oracle import ip_adapter_oracle
    import oracle.unet as ounet
    cfg, ocfg, sd, lat, pe, ne, emb = tiny
    plain_fn = ounet._attention
    with torch.no_grad():
        ref = unet_forward(sd, ocfg, lat, 501.0, pe)
        with ip_adapter_oracle(sd, emb, 0.0):
            zero = unet_forward(sd, ocfg, lat, 501.0, pe)
        with ip_adapter_oracle(sd, emb, 1.0):
            on = unet_forward(sd, ocfg, lat, 501.0, pe)
    assert ounet._attention is plain_fn                          # restored
    assert torch.equal(zero, ref)
    assert (on - ref).norm() / ref.norm() > 0.2


def test_oracle_equal_tokens_give_a_constant_row_whatever_q_is(tiny):
    """All T tokens of a sample equal: every softmax over them is uniform, so the image branch of a block is the constant
    row ``scale * W_o (W_v_ip tok)`` at every position.  Checked against that closed form in fp64."""
    import oracle.unet as ounet
    from tests.ip_adapter_oracle import ip_adapter_oracle
    cfg, ocfg, sd, lat, pe, ne, emb = tiny
    p = "down_blocks.1.attentions.0.transformer_blocks.0.attn2."
    c, cd, heads, scale = 128, cfg.cross_attention_dim, cfg.num_heads, 0.7
    g = torch.Generator().manual_seed(9)
    x = torch.randn(2, 16, c, generator=g)
    ctx = torch.randn(2, cfg.context_len, cd, generator=g)
    tok = torch.randn(2, 1, cd, generator=g).expand(2, IP_ADAPTER_TOKENS, cd).contiguous()
    plain = ounet._attention(sd, p, x, ctx, heads)
    with ip_adapter_oracle(sd, emb, scale) as toks:
        toks.copy_(tok)                                          # the closure's tokens, replaced by equal ones
        got = ounet._attention(sd, p, x, ctx, heads)
    wo, wv = sd[p + "to_out.0.weight"].double(), sd[p + "processor.to_v_ip.0.weight"].double()
    row = scale * (tok[:, 0].double() @ wv.t()) @ wo.t()         # [2, c]
    diff = (got - plain).double()
    assert torch.allclose(diff, row[:, None, :].expand_as(diff), rtol=0, atol=2e-5 * float(row.abs().max()) + 1e-6)
    assert float(row.abs().max()) > 1e-2


def test_oracle_negative_half_tokens_are_layernorm_of_the_bias(tiny):
    from tests.ip_adapter_oracle import cfg_image_embeds, ip_tokens
    cfg, ocfg, sd, lat, pe, ne, emb = tiny
    full = cfg_image_embeds(emb)
    assert full.shape == (4, E) and not full[:2].any() and torch.equal(full[2:], emb)
    toks = ip_tokens(sd, full)
    cd = cfg.cross_attention_dim
    want = F.layer_norm(sd[IP_PROJ + "image_embeds.bias"].view(IP_ADAPTER_TOKENS, cd), (cd,), sd[IP_PROJ + "norm.weight"],
                        sd[IP_PROJ + "norm.bias"], 1e-5)
    assert toks.shape == (4, IP_ADAPTER_TOKENS, cd)
    assert torch.equal(toks[0], want) and torch.equal(toks[1], want) and float(want.abs().max()) > 0.1
    # fp32 restatement of the projection against fp64
    w, b = sd[IP_PROJ + "image_embeds.weight"].double(), sd[IP_PROJ + "image_embeds.bias"].double()
    x = (emb.double() @ w.t() + b).view(2, IP_ADAPTER_TOKENS, cd)
    ref = F.layer_norm(x, (cd,), sd[IP_PROJ + "norm.weight"].double(), sd[IP_PROJ + "norm.bias"].double(), 1e-5)
    assert torch.allclose(toks[2:].double(), ref, rtol=0, atol=1e-4)


# ---------------------------------------------------------------------------------------------------------------------
# argument validation, on a model that never reaches a GPU
# ---------------------------------------------------------------------------------------------------------------------
def _model(key="stable_diffusion_model", **cfg_kw):
    from sonicdiffusionbayeslab_amd.registry import models_registry, schedulers_registry
    m = models_registry[key](unet_config=UNetConfig(sample_size=64, **cfg_kw), state_dict={})
    m.scheduler = schedulers_registry["ddim_scheduler"].from_config(m.scheduler.config)
    return m


def _no_gpu(model, monkeypatch):
    def boom(*a, **k):
        raise AssertionError("the arguments must be checked before the UNet is built")
    monkeypatch.setattr(model, "_ensure_unet", boom)


@pytest.mark.parametrize("key", ["stable_diffusion_model", "stable_diffusion_model_two_schedulers",
                                 "stable_diffusion_model_interliving_schedulers", "stable_diffusion_model_skip_timesteps"])
def test_image_prompt_arguments_are_checked_before_any_gpu_work(monkeypatch, key):
    from sonicdiffusionbayeslab_amd.registry import schedulers_registry
    model = _model(key)
    _no_gpu(model, monkeypatch)
    for a in ("scheduler_first", "scheduler_second", "scheduler_main", "scheduler_inter"):
        if hasattr(model, a):
            setattr(model, a, schedulers_registry["ddim_scheduler"].from_config(model.scheduler.config))
    pe = torch.zeros(2, 77, 768)
    call = lambda **kw: model(**{**dict(prompt_embeds=pe, negative_prompt_embeds=pe, output_type="latent"), **kw})
    e = model.IP_ADAPTER_EMBED_DIM
    emb = torch.zeros(2, e)
    with pytest.raises(ValueError, match="need a loaded IP-Adapter"):
        call(ip_adapter_image_embeds=emb)
    with pytest.raises(ValueError, match="need a loaded IP-Adapter"):
        call(ip_adapter_image=torch.zeros(2, 3, 32, 32, dtype=torch.uint8))
    model.load_ip_adapter("h94/IP-Adapter", subfolder="models", weight_name="ip-adapter_sd15.bin")
    assert "SYNTHETIC stand-in for the hub IP-Adapter h94/IP-Adapter" in model.weights_source
    assert model.unet_config.ip_adapter_embed_dim == e and len(model._ip_sd) == 36
    with pytest.raises(ValueError, match="exclusive"):
        call(ip_adapter_image_embeds=emb, ip_adapter_image=torch.zeros(2, 3, 32, 32, dtype=torch.uint8))
    with pytest.raises(ValueError, match=rf"E = {e}"):
        call(ip_adapter_image_embeds=torch.zeros(2, 768))
    with pytest.raises(ValueError, match="does not match the prompt batch"):
        call(ip_adapter_image_embeds=torch.zeros(3, e))
    with pytest.raises(NotImplementedError, match="several IP-Adapters"):
        call(ip_adapter_image_embeds=[emb, emb])
    with pytest.raises(NotImplementedError, match="several images per sample"):
        call(ip_adapter_image_embeds=torch.zeros(2, 3, e))
    with pytest.raises(ValueError, match="image encoder"):          # a hub stand-in has no local image_encoder
        call(ip_adapter_image=torch.zeros(2, 3, 32, 32, dtype=torch.uint8))
    with pytest.raises(NotImplementedError, match="nested lists"):
        call(ip_adapter_image=[[torch.zeros(3, 8, 8)]])
    # the accepted forms reach the UNet build: [B, E], [B, 1, E], a one-element list, [2 B, E] under CFG, a batch of 1
    for ok in (emb, emb[:, None], [emb], torch.zeros(4, e), torch.zeros(1, e), torch.zeros(4, 1, e)):
        with pytest.raises(AssertionError, match="before the UNet is built"):
            call(ip_adapter_image_embeds=ok)
    with pytest.raises(ValueError, match="does not match the prompt batch"):   # 2 B rows mean negative | positive only under CFG
        call(ip_adapter_image_embeds=torch.zeros(4, e), guidance_scale=1.0)
    with pytest.raises(NotImplementedError, match="per-block"):
        model.set_ip_adapter_scale({"down": 1.0})
    with pytest.raises(ValueError, match="finite"):
        model.set_ip_adapter_scale(float("nan"))
    model.set_ip_adapter_scale(0.5)
    assert model._ip_scale == 0.5
    with pytest.raises(NotImplementedError, match="already loaded"):
        model.load_ip_adapter("h94/IP-Adapter", subfolder="models", weight_name="ip-adapter_sd15.bin")
    with pytest.raises(NotImplementedError, match="several IP-Adapters"):
        _model().load_ip_adapter(["a", "b"], subfolder=["m", "m"], weight_name=["x.bin", "y.bin"])
    model.unload_ip_adapter()
    assert model.unet_config.ip_adapter_embed_dim is None and model._ip_sd is None
    with pytest.raises(ValueError, match="need a loaded IP-Adapter"):
        call(ip_adapter_image_embeds=emb)


def test_embeds_halves_and_broadcast():
    model = _model()
    model.load_ip_adapter("h94/IP-Adapter", weight_name="ip-adapter_sd15.bin")
    e = model.IP_ADAPTER_EMBED_DIM
    full = torch.arange(4 * e, dtype=torch.float32).view(4, e)
    kind, pos, neg = model._ip_adapter_args(None, full, 2, True)
    assert kind == "embeds" and torch.equal(pos, full[2:]) and torch.equal(neg, full[:2])
    kind, pos, neg = model._ip_adapter_args(None, [full[:2, None]], 2, True)
    assert neg is None and torch.equal(pos, full[:2])
    kind, pos, neg = model._ip_adapter_args(None, full[:1], 3, False)
    assert neg is None and pos.shape == (3, e) and torch.equal(pos[2], full[0])
    assert model._ip_adapter_args(None, None, 2, True) is None


def test_local_adapter_directory_and_image_encoder_checks(tmp_path):
    import json
    base = UNetConfig(sample_size=64, **{k: v for k, v in TINY.items() if k != "sample_size"})
    cfg = dataclasses.replace(base, ip_adapter_embed_dim=E)
    sd = make_synthetic_ip_adapter_state_dict(cfg, seed=3)
    (tmp_path / "models" / "image_encoder").mkdir(parents=True)
    torch.save(to_upstream_ip_adapter(sd, cfg), str(tmp_path / "models" / "ip-adapter_sd15.bin"))
    enc = dict(hidden_size=1280, num_hidden_layers=2, num_attention_heads=16, intermediate_size=5120, image_size=224, patch_size=14,
               projection_dim=E, hidden_act="gelu")
    (tmp_path / "models" / "image_encoder" / "config.json").write_text(json.dumps(enc))
    from sonicdiffusionbayeslab_amd.models import StableDiffusionModel
    m = StableDiffusionModel(unet_config=base, state_dict={})
    with pytest.raises(ValueError, match="weight_name"):
        m.load_ip_adapter(str(tmp_path), subfolder="models")
    with pytest.raises(FileNotFoundError):
        m.load_ip_adapter(str(tmp_path), subfolder="models", weight_name="missing.bin")
    m.load_ip_adapter(str(tmp_path), subfolder="models", weight_name="ip-adapter_sd15.bin")
    assert "IP-Adapter(local:" in m.weights_source and m.unet_config.ip_adapter_embed_dim == E
    assert all(torch.equal(m._ip_sd[k], sd[k]) for k in sd)
    img = torch.zeros(1, 3, 32, 32, dtype=torch.uint8)
    # the published encoder's shape (ViT-H/14: head dim 80, exact gelu) is built by the HIP tower ...
    assert m._ip_adapter_args(img, None, 1, True)[0] == "image"
    assert m._ip_image_encoder_config().hidden_act == "gelu"
    # ... other activations and head dims are refused by name, on the host
    enc.update(hidden_act="relu")
    (tmp_path / "models" / "image_encoder" / "config.json").write_text(json.dumps(enc))
    with pytest.raises(NotImplementedError, match="hidden_act='relu'"):
        m._ip_adapter_args(img, None, 1, True)
    enc.update(hidden_act="quick_gelu", num_attention_heads=10)
    (tmp_path / "models" / "image_encoder" / "config.json").write_text(json.dumps(enc))
    with pytest.raises(NotImplementedError, match="head dim 64"):
        m._ip_adapter_args(img, None, 1, True)
    enc.update(hidden_size=128, num_attention_heads=2, intermediate_size=256, projection_dim=64)
    (tmp_path / "models" / "image_encoder" / "config.json").write_text(json.dumps(enc))
    with pytest.raises(ValueError, match="projects to 64"):
        m._ip_adapter_args(img, None, 1, True)
    enc.update(projection_dim=E)
    (tmp_path / "models" / "image_encoder" / "config.json").write_text(json.dumps(enc))
    kind, got = m._ip_adapter_args(torch.full((1, 3, 32, 32), 0.5), None, 2, True)          # floats in [0, 1], batch 1 broadcast
    assert kind == "image" and got.dtype == torch.uint8 and got.shape == (2, 3, 32, 32) and int(got[1, 0, 0, 0]) == 128
    from PIL import Image
    kind, got = m._ip_adapter_args([Image.new("RGB", (24, 16), (255, 0, 7))] * 2, None, 2, False)
    assert got.shape == (2, 3, 16, 24) and got[0, :, 0, 0].tolist() == [255, 0, 7]


def test_unet_wrapper_refuses_other_added_cond_kwargs_without_a_gpu():
    from sonicdiffusionbayeslab_amd.unet import HipUNet2DConditionModel
    net = HipUNet2DConditionModel.__new__(HipUNet2DConditionModel)
    net.config = UNetConfig(sample_size=16)
    x, ctx = torch.zeros(1, 4, 16, 16), torch.zeros(1, 77, 768)
    for kw in ({}, {"image_embeds": torch.zeros(1, E)}, {"text_embeds": None}):
        with pytest.raises(NotImplementedError, match="no IP-Adapter"):
            net(x, 1, encoder_hidden_states=ctx, added_cond_kwargs=kw)
    net.config = UNetConfig(sample_size=16, ip_adapter_embed_dim=E)
    for kw in ({}, {"text_embeds": None}, {"image_embeds": torch.zeros(1, E), "time_ids": None}):
        with pytest.raises(NotImplementedError, match="only"):
            net(x, 1, encoder_hidden_states=ctx, added_cond_kwargs=kw)
    with pytest.raises(NotImplementedError, match="several IP-Adapters"):
        net(x, 1, encoder_hidden_states=ctx, added_cond_kwargs={"image_embeds": [torch.zeros(1, E)] * 2})
    with pytest.raises(NotImplementedError, match="several images"):
        net(x, 1, encoder_hidden_states=ctx, added_cond_kwargs={"image_embeds": torch.zeros(1, 2, E)})
    with pytest.raises(ValueError, match="image_embeds must be"):
        net(x, 1, encoder_hidden_states=ctx, added_cond_kwargs={"image_embeds": torch.zeros(1, 2 * E)})
    net._handle = None                                           # (nothing to destroy)


def test_shard_slices_ride_with_the_prompts():
    from sonicdiffusionbayeslab_amd import dist as sdist
    from sonicdiffusionbayeslab_amd.models import StableDiffusionModel
    n = 5
    emb = torch.arange(n, dtype=torch.float32)[:, None].repeat(1, 8)
    both = torch.cat([emb + 100, emb])                           # [negative | positive]
    img = torch.arange(n, dtype=torch.uint8)[:, None, None, None].expand(n, 3, 4, 4)
    seen = []
    for rank in range(2):
        lo, hi = sdist.shard_range(n, rank, 2)
        kw = StableDiffusionModel.shard_ip_adapter_args({"ip_adapter_image_embeds": emb, "num_inference_steps": 3}, lo, hi, n)
        assert kw["num_inference_steps"] == 3 and kw["ip_adapter_image_embeds"][:, 0].tolist() == list(range(lo, hi))
        seen += kw["ip_adapter_image_embeds"][:, 0].tolist()
        kw = StableDiffusionModel.shard_ip_adapter_args({"ip_adapter_image_embeds": [both]}, lo, hi, n)
        assert kw["ip_adapter_image_embeds"][0][:, 0].tolist() == [100 + i for i in range(lo, hi)] + list(range(lo, hi))
        kw = StableDiffusionModel.shard_ip_adapter_args({"ip_adapter_image": img}, lo, hi, n)
        assert kw["ip_adapter_image"][:, 0, 0, 0].tolist() == list(range(lo, hi))
        kw = StableDiffusionModel.shard_ip_adapter_args({"ip_adapter_image": list(range(n))}, lo, hi, n)
        assert kw["ip_adapter_image"] == list(range(lo, hi))
        kw = StableDiffusionModel.shard_ip_adapter_args({"ip_adapter_image_embeds": emb[:1]}, lo, hi, n)     # a batch of 1 is broadcast
        assert kw["ip_adapter_image_embeds"].shape[0] == 1
    assert seen == list(range(n))


# ---------------------------------------------------------------------------------------------------------------------
# the operator test's bound discriminates (tests/ip_xattn_case.py): no GPU needed to know that
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("UB,rps,C,heads", IP_XATTN_SHAPES)
def test_operator_bound_is_small_beside_the_branch_and_wrong_kernels_violate_it(UB, rps, C, heads):
    """On the ``sharp`` operands the a-priori bound is a small fraction of the image branch (median bound <= a tenth of the
    branch's rms), and a kernel that is wrong in one way -- no branch, the branch scaled, a uniform softmax, gamma or beta
    dropped, another sample's operands -- violates it in at least a quarter of all elements.  The thresholds are a tenth and
    a quarter because a check is only worth its name if an error of the size of the effect fails it broadly, not in a lucky
    element; they are not fitted (the figures are printed)."""
    ops = operands(UB, rps, C, heads, "sharp")
    y, bound, branch = ref_bound(*ops, EPS, UB, rps, C, heads)
    rms = branch.pow(2).mean().sqrt().item()
    print(f"sharp UB={UB} rows={rps} C={C} heads={heads}: branch rms {rms:.3f}, bound median {bound.median().item():.4f} max {bound.max().item():.4f}")
    assert bound.median().item() <= 0.1 * rms
    for name, wrong in perturbed(*ops, EPS, UB, rps, C, heads).items():
        frac = ((wrong - y).abs() > bound).double().mean().item()
        print(f"  {name}: violates {100 * frac:.1f} % of elements")
        assert frac >= 0.25, name


def test_mistyped_local_paths_raise_and_unload_restores_weights_source(tmp_path):
    """Only ``name`` / ``org/name`` counts as a hub name (and gets the seeded stand-in); a path that is absolute, relative
    with dots, deeper than one separator or ends like a weight file, and does not exist, raises instead of loading random
    weights.  ``unload_ip_adapter`` takes the adapter's note off ``weights_source`` again."""
    from sonicdiffusionbayeslab_amd.models import StableDiffusionModel
    base = UNetConfig(sample_size=64, **{k: v for k, v in TINY.items() if k != "sample_size"})
    m = StableDiffusionModel(unet_config=base, state_dict={})
    before = m.weights_source
    for wrong in (str(tmp_path / "no_such_dir"), str(tmp_path / "no_such_dir" / "ip-adapter_sd15.bin"), "./adapters/ip", "../ip",
                  "a/b/c", "ip-adapter_sd15.safetensors", "~/adapters"):
        with pytest.raises(FileNotFoundError):
            m.load_ip_adapter(wrong, subfolder="models", weight_name="ip-adapter_sd15.bin")
        assert m.weights_source == before and not m._ip_loaded
    m.load_ip_adapter("h94/IP-Adapter", subfolder="models", weight_name="ip-adapter_sd15.bin")
    assert m.weights_source.startswith(before) and "SYNTHETIC stand-in" in m.weights_source[len(before):]
    m.unload_ip_adapter()
    assert m.weights_source == before

