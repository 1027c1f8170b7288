"""CLIP score, host side: Pillow-exact tap tables of the preprocessing, the fp32 vision / score oracle against transformers,
the new C ABI symbols and the config checks of HipClipScorer.from_pretrained."""
import json
import os

import numpy as np
import pytest
import torch

from tests.clip_score_util import PROMPTS, tiny_images, tiny_state_dict, write_tiny_clip_dir
from tests.clip_vision_oracle import (clip_scores, clip_text_embeds, clip_vision_forward, pil_crop, pixel_values,
                                      resize_geometry)

TAP_SIZES = [(512, 512), (512, 768), (768, 512), (1024, 1024), (224, 224), (100, 150), (37, 53), (1, 1)]


def taps(lib, n_in, n_out, first, count):
    import ctypes as C
    ks = lib.sd_clip_resize_taps(n_in, n_out, first, count, None, None, None)
    assert ks > 0
    xmin, xcnt = np.zeros(count, np.int32), np.zeros(count, np.int32)
    k = np.zeros((count, ks), np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    assert lib.sd_clip_resize_taps(n_in, n_out, first, count, p(xmin), p(xcnt), p(k)) == ks
    return xmin, xcnt, k


def apply_taps(a, xmin, xcnt, k, axis):
    """Pillow's 8-bpc pass along ``axis`` of an int array: 2^21 + sum(pixel * coeff), >> 22, clipped to [0, 255]."""
    a = np.moveaxis(a.astype(np.int64), axis, -1)
    out = np.empty(a.shape[:-1] + (len(xmin),), np.int64)
    for i in range(len(xmin)):
        s = np.full(a.shape[:-1], 1 << 21, np.int64)
        for j in range(xcnt[i]):
            s += a[..., xmin[i] + j] * int(k[i, j])
        out[..., i] = np.clip(s >> 22, 0, 255)
    return np.moveaxis(out, -1, axis)


@pytest.mark.parametrize("h,w", TAP_SIZES)
def test_tap_tables_reproduce_pil_bicubic_and_crop(sdlib, h, w):
    """Horizontal pass over the rows the crop's vertical taps read, then the vertical pass: equal to PIL bit for bit."""
    g = torch.Generator().manual_seed(h * 7919 + w)
    img = torch.randint(0, 256, (3, h, w), generator=g, dtype=torch.uint8)
    S = 224
    rh, rw, top, left = resize_geometry(h, w, S)
    xmin, xcnt, xk = taps(sdlib, w, rw, left, S)
    ymin, ycnt, yk = taps(sdlib, h, rh, top, S)
    y0, y1 = int(ymin.min()), int((ymin + ycnt).max())
    mid = apply_taps(img.numpy()[:, y0:y1, :], xmin, xcnt, xk, axis=2)          # [3, rows, S] uint8 intermediate
    got = apply_taps(mid, ymin - y0, ycnt, yk, axis=1)
    want = pil_crop(img, S).numpy()
    assert got.shape == want.shape == (3, S, S)
    assert np.array_equal(got, want), f"{h}x{w}: {(got != want).sum()} pixels differ"
    assert xk.sum(1).min() > 0 and ycnt.max() <= yk.shape[1]


def test_tap_table_refuses_a_bad_window(sdlib):
    assert sdlib.sd_clip_resize_taps(100, 224, 200, 100, None, None, None) < 0


def test_new_abi_symbols_load(sdlib):
    for n in ("sd_clip_vision_create", "sd_clip_vision_workspace_bytes", "sd_clip_vision_encode", "sd_clip_create_projected",
              "sd_clip_text_embeds", "sd_clip_text_embeds_workspace_bytes", "sd_clip_score", "sd_clip_resize_taps",
              "sd_op_vit_attention", "sd_op_clip_preprocess"):
        assert getattr(sdlib, n) is not None


def test_vision_parameter_enumeration_matches_transformers_names(sdlib):
    """The kind-3 handle enumerates the CLIPVisionModelWithProjection names (pre_layrnorm spelling included) with their shapes;
    creating a handle needs no GPU."""
    import ctypes as C
    from sonicdiffusionbayeslab_amd import _lib
    from sonicdiffusionbayeslab_amd.clip_score import ClipVisionConfig, clip_vision_param_shapes
    cfg = ClipVisionConfig(num_hidden_layers=2, patch_size=14, projection_dim=768, hidden_size=1024, num_attention_heads=16,
                           intermediate_size=4096)
    h = C.c_void_p()
    c = _lib.SdClipVisionConfig(1024, 2, 16, 4096, 224, 14, 768, 1e-5)
    _lib.check(sdlib.sd_clip_vision_create(C.byref(c), C.byref(h)))
    try:
        got = []
        for i in range(sdlib.sd_unet_num_params(h)):
            name = C.create_string_buffer(256)
            shape = (C.c_longlong * 4)()
            nd = C.c_int()
            _lib.check(sdlib.sd_unet_param_info(h, i, name, 256, shape, C.byref(nd)))
            got.append((name.value.decode(), tuple(shape[:nd.value])))
        assert got == clip_vision_param_shapes(cfg)
    finally:
        sdlib.sd_unet_destroy(h)
    bad = _lib.SdClipVisionConfig(1024, 2, 8, 4096, 224, 14, 768, 1e-5)          # head dim 128
    assert sdlib.sd_clip_vision_create(C.byref(bad), C.byref(h)) != 0
    assert b"head dim" in sdlib.sd_last_error()
    bad = _lib.SdClipVisionConfig(768, 2, 12, 3072, 336, 14, 768, 1e-5)          # 577 tokens
    assert sdlib.sd_clip_vision_create(C.byref(bad), C.byref(h)) != 0


def test_oracle_reproduces_transformers_vision_tower_and_metric(tmp_path):
    pytest.importorskip("transformers")
    from transformers import CLIPVisionModelWithProjection
    from sonicdiffusionbayeslab_amd.metrics import ClipScoreMetric
    from tests.clip_score_util import tiny_configs
    d = write_tiny_clip_dir(str(tmp_path / "clip"))
    tcfg, vcfg = tiny_configs()
    sd = tiny_state_dict()
    images = tiny_images()
    m = ClipScoreMetric(d, backend="transformers")
    inp = m.processor(text=PROMPTS, images=images, return_tensors="pt", padding=True, truncation=True)
    pix = torch.stack([pixel_values(pil_crop(im, 224)) for im in images])
    assert (pix - inp["pixel_values"]).abs().max().item() < 1e-5
    vm = CLIPVisionModelWithProjection.from_pretrained(d).eval()
    with torch.no_grad():
        want = vm(pixel_values=inp["pixel_values"]).image_embeds
    got = clip_vision_forward(sd, vcfg, pix)
    assert ((got - want).norm() / want.norm()).item() < 1e-5
    # the whole metric: oracle text embeddings (EOS pooling) and per-pair scores vs ClipScoreMetric's transformers path
    from sonicdiffusionbayeslab_amd.clip import ClipBpeTokenizer
    tok = ClipBpeTokenizer.from_pretrained(d, model_max_length=tcfg.max_position_embeddings)
    ids = tok(PROMPTS)
    cfgj = json.load(open(os.path.join(d, "config.json")))
    eos = cfgj["text_config"]["eos_token_id"]
    txt = clip_text_embeds(sd, tcfg, ids, None if eos == 2 else eos)
    raw = clip_scores(got, txt)
    m.reset()
    for s in range(0, len(images), 2):
        m.update(torch.stack(images[s:s + 2]), PROMPTS[s:s + 2])
    assert abs(raw.clamp(min=0).mean().item() - float(m.compute())) < 1e-3
    gold = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "clip_score_golden.json")))
    assert torch.allclose(raw.float(), torch.tensor(gold["raw_scores"]), atol=1e-3)


def _edit_config(d, section, **kw):
    p = os.path.join(d, "config.json")
    j = json.load(open(p))
    (j[section] if section else j).update(kw)
    json.dump(j, open(p, "w"))


@pytest.mark.parametrize("section,field,value", [
    ("vision_config", "hidden_act", "gelu"), ("text_config", "hidden_act", "gelu"),
    ("vision_config", "num_attention_heads", 4), ("vision_config", "image_size", 336),
    ("vision_config", "hidden_size", 2048), ("vision_config", "layer_norm_eps", 1e-6), (None, "projection_dim", 66)])
def test_from_pretrained_refuses_unsupported_configs(tmp_path, section, field, value):
    from sonicdiffusionbayeslab_amd.clip_score import HipClipScorer
    d = write_tiny_clip_dir(str(tmp_path / "clip"))
    _edit_config(d, section, **{field: value})
    with pytest.raises(ValueError, match=field):
        HipClipScorer.from_pretrained(d)


def test_from_pretrained_refuses_other_preprocessing(tmp_path):
    from sonicdiffusionbayeslab_amd.clip_score import HipClipScorer
    d = write_tiny_clip_dir(str(tmp_path / "clip"))
    p = os.path.join(d, "preprocessor_config.json")
    j = json.load(open(p))
    j["resample"] = 2
    json.dump(j, open(p, "w"))
    with pytest.raises(ValueError, match="resample"):
        HipClipScorer.from_pretrained(d)


def test_metric_refuses_unknown_backend(tmp_path):
    from sonicdiffusionbayeslab_amd.metrics import ClipScoreMetric
    with pytest.raises(ValueError, match="backend"):
        ClipScoreMetric(str(tmp_path), backend="onnx")


def test_tokenizer_ids_equal_the_transformers_golden(tmp_path):
    """ClipBpeTokenizer on the tiny checkpoint gives transformers' CLIPProcessor ids (recorded with padding=True, i.e. to
    the longest prompt); past that length the scorer pads with the pad token, up to max_position_embeddings."""
    from sonicdiffusionbayeslab_amd.clip import ClipBpeTokenizer
    gold = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "clip_score_golden.json")))
    d = write_tiny_clip_dir(str(tmp_path / "clip"))
    tok = ClipBpeTokenizer.from_pretrained(d, model_max_length=16)
    ids = tok(gold["prompts"])
    want = torch.tensor(gold["input_ids"])
    n = want.shape[1]
    assert torch.equal(ids[:, :n], want.to(ids.dtype))
    assert (ids[:, n:] == tok.pad_token_id).all()


def test_hip_metric_checks_config_at_construction_and_defers_gpu_work(tmp_path, monkeypatch):
    """backend="hip" refuses an unsupported checkpoint when the metric is built; a supported one builds no tower (and
    touches no device) until the first update."""
    from sonicdiffusionbayeslab_amd.metrics import ClipScoreMetric
    d = write_tiny_clip_dir(str(tmp_path / "clip"))
    import sonicdiffusionbayeslab_amd.clip_score as cs

    def no_gpu(*a, **k):
        raise AssertionError("GPU work while building the metric")
    monkeypatch.setattr(cs.HipClipScorer, "from_pretrained", no_gpu)
    monkeypatch.setattr(torch.cuda, "set_device", no_gpu)
    m = ClipScoreMetric(d, backend="hip", device="cuda:1")
    assert m.scorer is None and m.device == "cuda:1"
    _edit_config(d, "vision_config", hidden_act="gelu")
    with pytest.raises(ValueError, match="hidden_act"):
        ClipScoreMetric(d, backend="hip")


def test_missing_eos_token_id_takes_the_transformers_default(tmp_path):
    from sonicdiffusionbayeslab_amd.clip_score import read_clip_configs
    pytest.importorskip("transformers")
    from transformers import CLIPTextConfig
    d = write_tiny_clip_dir(str(tmp_path / "clip"))
    p = os.path.join(d, "config.json")
    j = json.load(open(p))
    del j["text_config"]["eos_token_id"]
    json.dump(j, open(p, "w"))
    _, _, eos = read_clip_configs(d)
    assert eos == CLIPTextConfig().eos_token_id != 2
