"""LCM-distilled UNets (diffusers ``time_cond_proj_dim``), host side: config loading, parameter enumeration in Python and in
libsdhip, the synthetic ``cond_proj`` weight, the guidance-scale embedding against a float64 evaluation of its formula, and
the pipeline / harness wiring that runs without a GPU.  Reference call sites: src/models.py:195-202,231."""
import ctypes as C
import json
import math
import os

import pytest
import torch

from sonicdiffusionbayeslab_amd import _lib
from sonicdiffusionbayeslab_amd.models import StableDiffusionModel
from sonicdiffusionbayeslab_amd.weights import UNetConfig, load_unet_config, make_synthetic_state_dict, param_shapes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the loader as the package defines it, taken at collection time: a test that runs the harness in-process may replace
# StableDiffusionModel.from_pretrained with a stand-in for the rest of the session (tests/test_dist_gpu.py does)
_FROM_PRETRAINED = StableDiffusionModel.__dict__["from_pretrained"]


@pytest.fixture
def real_from_pretrained(monkeypatch):
    monkeypatch.setattr(StableDiffusionModel, "from_pretrained", _FROM_PRETRAINED)
    monkeypatch.delenv("SD_AMD_MODEL_DIR", raising=False)
COND = "time_embedding.cond_proj.weight"
TINY = dict(sample_size=8, block_out_channels=(320, 640), attn_levels=(True, False))


def _write_unet_config(root, **extra):
    os.makedirs(os.path.join(root, "unet"), exist_ok=True)
    c = {"sample_size": 64, "block_out_channels": [320, 640, 1280, 1280], "attention_head_dim": 8,
         "down_block_types": ["CrossAttnDownBlock2D"] * 3 + ["DownBlock2D"],
         "up_block_types": ["UpBlock2D"] + ["CrossAttnUpBlock2D"] * 3, **extra}
    with open(os.path.join(root, "unet", "config.json"), "w") as f:
        json.dump(c, f)


def test_load_unet_config_accepts_a_positive_time_cond_proj_dim(tmp_path):
    _write_unet_config(str(tmp_path), time_cond_proj_dim=256)
    cfg = load_unet_config(str(tmp_path))
    assert cfg.time_cond_proj_dim == 256 and cfg == UNetConfig(time_cond_proj_dim=256)
    assert cfg != UNetConfig()
    _write_unet_config(str(tmp_path), time_cond_proj_dim=None)
    assert load_unet_config(str(tmp_path)).time_cond_proj_dim is None
    for bad in (0, -8, "256", 2.5):
        _write_unet_config(str(tmp_path), time_cond_proj_dim=bad)
        with pytest.raises(NotImplementedError):
            load_unet_config(str(tmp_path))
    # every other key check stays
    _write_unet_config(str(tmp_path), time_cond_proj_dim=256, class_embed_type="timestep")
    with pytest.raises(NotImplementedError):
        load_unet_config(str(tmp_path))


def test_config_value_survives_replace_and_stays_out_of_asdict():
    import dataclasses

    from oracle.unet import UNetConfig as OC
    cfg = UNetConfig(sample_size=16, time_cond_proj_dim=256)
    assert dataclasses.replace(cfg, sample_size=32).time_cond_proj_dim == 256
    assert "time_cond_proj_dim" not in dataclasses.asdict(cfg)
    OC(**dataclasses.asdict(cfg))              # the oracle's config is still built from the dict
    with pytest.raises(ValueError):
        UNetConfig(time_cond_proj_dim=0)


def test_param_shapes_gain_exactly_cond_proj():
    plain = param_shapes(UNetConfig())
    cond = param_shapes(UNetConfig(time_cond_proj_dim=256))
    assert len(plain) == 686 and len(cond) == 687 and COND not in dict(plain)
    assert dict(cond)[COND] == (320, 256)
    assert [p for p in cond if p[0] != COND] == plain
    assert param_shapes(UNetConfig(time_cond_proj_dim=None)) == plain


def test_synthetic_shared_weights_are_bit_identical_to_the_plain_config():
    plain = make_synthetic_state_dict(UNetConfig(**TINY), seed=5)
    cond = make_synthetic_state_dict(UNetConfig(**TINY, time_cond_proj_dim=256), seed=5)
    assert set(cond) == set(plain) | {COND}
    for k, v in plain.items():
        assert torch.equal(cond[k], v), k
    w = cond[COND]
    assert w.shape == (320, 256) and torch.equal(w, w.bfloat16().float())
    assert 0.03 < w.std().item() < 0.1                       # ~ N(0, 1/256)
    again = make_synthetic_state_dict(UNetConfig(**TINY, time_cond_proj_dim=256), seed=5)
    assert torch.equal(again[COND], w)
    assert not torch.equal(make_synthetic_state_dict(UNetConfig(**TINY, time_cond_proj_dim=256), seed=6)[COND], w)


def _create(lib, cfg):
    from sonicdiffusionbayeslab_amd.unet import _c_config
    h = C.c_void_p()
    rc = lib.sd_unet_create(C.byref(_c_config(cfg)), C.byref(h))
    return rc, h


def test_library_enumerates_and_loads_cond_proj_only_when_configured():
    lib = _lib.load()
    cfg = UNetConfig(time_cond_proj_dim=256)
    rc, h = _create(lib, cfg)
    assert rc == 0, lib.sd_last_error()
    shapes = param_shapes(cfg)
    assert lib.sd_unet_num_params(h) == len(shapes) == 687
    name = C.create_string_buffer(256); shp = (C.c_longlong * 4)(); nd = C.c_int()
    for i, (n, s) in enumerate(shapes):
        _lib.check(lib.sd_unet_param_info(h, i, name, 256, shp, C.byref(nd)))
        assert name.value.decode() == n and tuple(shp[: nd.value]) == tuple(s), (i, n)
    w = torch.zeros(320 * 256)
    _lib.check(lib.sd_unet_load_param(h, COND.encode(), w.data_ptr(), w.numel()))
    assert lib.sd_unet_load_param(h, COND.encode(), w.data_ptr(), 320 * 128) != 0          # wrong shape
    assert b"expects 81920 elements" in lib.sd_last_error()
    lib.sd_unet_destroy(h)
    rc, h = _create(lib, UNetConfig())
    assert rc == 0
    assert lib.sd_unet_num_params(h) == 686
    assert lib.sd_unet_load_param(h, COND.encode(), w.data_ptr(), w.numel()) != 0
    assert b"unknown parameter" in lib.sd_last_error()
    # the forward-side entry point: a plain handle has nothing to condition, NULL (clear) is always accepted
    cond = torch.zeros(256)
    assert lib.sd_unet_set_timestep_cond(h, None, cond.data_ptr()) != 0
    assert b"no time_embedding.cond_proj" in lib.sd_last_error()
    assert lib.sd_unet_set_timestep_cond(h, None, None) == 0
    lib.sd_unet_destroy(h)
    for bad in (12, 100):                                   # the GEMV reads 8 bf16 at a time
        rc, h = _create(lib, UNetConfig(time_cond_proj_dim=bad))
        assert rc != 0 and b"multiple of 8" in lib.sd_last_error()


def test_load_params_checks_the_cond_proj_shape():
    from sonicdiffusionbayeslab_amd.unet import load_params
    lib = _lib.load()
    cfg = UNetConfig(**TINY, time_cond_proj_dim=256)
    sd = make_synthetic_state_dict(cfg, seed=5)
    rc, h = _create(lib, cfg)
    assert rc == 0
    bad = dict(sd); bad[COND] = sd[COND].t().contiguous()                 # [256, 320]: same numel, wrong shape
    with pytest.raises(ValueError):
        load_params(lib, h, cfg, bad)
    bad.pop(COND)
    with pytest.raises(KeyError):
        load_params(lib, h, cfg, bad)
    load_params(lib, h, cfg, sd)
    if not torch.cuda.is_available():                      # packed on the host, then no device to upload to
        assert lib.sd_unet_finalize(h) == -2 and b"hipMalloc" in lib.sd_last_error()
        buf = torch.empty(320 * 256, dtype=torch.bfloat16)
        assert lib.sd_unet_debug_packed(h, COND.encode(), buf.data_ptr(), buf.numel() * 2) >= 0
        assert torch.equal(buf.float().view(320, 256), sd[COND])     # bf16 [320][256], the gemv_kernel layout of linear_1
    lib.sd_unet_destroy(h)


def _embedding_f64(w, d):
    half = d // 2
    k = torch.arange(half, dtype=torch.float64)
    a = (float(w) * 1000.0) * torch.exp(-k * math.log(10000.0) / (half - 1))
    out = torch.cat([torch.sin(a), torch.cos(a)])
    if d % 2:
        out = torch.cat([out, torch.zeros(1, dtype=torch.float64)])
    return out, torch.cat([a, a, torch.zeros(d % 2, dtype=torch.float64)])


@pytest.mark.parametrize("d", [256, 255, 17])
def test_guidance_scale_embedding_matches_float64_formula(d):
    from sonicdiffusionbayeslab_amd.models import get_guidance_scale_embedding
    ws = [-1.0, 0.0, 7.0]
    got = get_guidance_scale_embedding(torch.tensor(ws), d)
    assert got.shape == (3, d) and got.dtype == torch.float32
    for i, w in enumerate(ws):
        want, angle = _embedding_f64(w, d)
        # fp32: the frequency carries ~(ln 1e4 + 3) ulp of relative error, the angle one more rounding, sin / cos ~1 ulp
        bound = angle.abs() * 16 * 2.0 ** -24 + 4 * 2.0 ** -24
        err = (got[i].double() - want).abs()
        assert (err <= bound).all(), (w, (err - bound).max().item())
    if d % 2:
        assert (got[:, -1] == 0).all()
    # w = 0: [0 ... | 1 ...]; the layout is [sin | cos], not the timestep sinusoid's [cos | sin]
    assert (got[1, : d // 2] == 0).all() and (got[1, d // 2: 2 * (d // 2)] == 1).all()
    assert torch.equal(get_guidance_scale_embedding(7.0, d)[0], got[2])


def test_no_classifier_free_guidance_for_a_guidance_conditioned_unet():
    from sonicdiffusionbayeslab_amd.models import StableDiffusionModel, get_guidance_scale_embedding
    m = StableDiffusionModel(unet_config=UNetConfig(time_cond_proj_dim=256))
    m._guidance_scale = 8.0
    assert not m.do_classifier_free_guidance
    assert torch.equal(m.guidance_condition(8.0), get_guidance_scale_embedding(7.0, 256))
    plain = StableDiffusionModel(unet_config=UNetConfig())
    plain._guidance_scale = 8.0
    assert plain.do_classifier_free_guidance and plain.guidance_condition(8.0) is None


def test_from_pretrained_time_cond_proj_dim(tmp_path, real_from_pretrained):
    m = StableDiffusionModel.from_pretrained("SimianLuo/LCM_Dreamshaper_v7", time_cond_proj_dim=256)
    assert m.unet_config.time_cond_proj_dim == 256 and m.weights_source.startswith("synthetic(")
    assert StableDiffusionModel.from_pretrained("Lykon/dreamshaper-7").unet_config.time_cond_proj_dim is None
    # a local checkpoint's unet/config.json decides; a different YAML value is an error
    _write_unet_config(str(tmp_path), time_cond_proj_dim=256)
    ucfg = load_unet_config(str(tmp_path))
    assert ucfg.time_cond_proj_dim == 256
    with pytest.raises(ValueError, match="conflicts"):
        StableDiffusionModel.from_pretrained(str(tmp_path), time_cond_proj_dim=128)
    _write_unet_config(str(tmp_path))
    with pytest.raises(ValueError, match="conflicts"):
        StableDiffusionModel.from_pretrained(str(tmp_path), time_cond_proj_dim=256)


def _method(config_name):
    from sonicdiffusionbayeslab_amd.config import load_named_config
    from sonicdiffusionbayeslab_amd.experiments.consistency_model import ConsistencyModelMethod
    m = ConsistencyModelMethod.__new__(ConsistencyModelMethod)     # the hooks alone: no process group, no GPU
    m.config = load_named_config(config_name, os.path.join(ROOT, "configs"))
    m.device = "cpu"
    m.setup_exp_params()
    m.setup_model()
    return m


def test_lcm_distilled_config_runs_the_consistency_method_without_a_lora(real_from_pretrained):
    m = _method("lcm_distilled_config.yaml")
    c = m.config
    assert c.experiment.method == "consistency_model" and c.scheduler.scheduler_name == "lcm_scheduler"
    assert c.model.pretrained_model == "SimianLuo/LCM_Dreamshaper_v7"
    assert c.experiment_params.guidance_scale == 8.0 and c.experiment_params.num_inference_steps == [1, 2, 4, 8]
    assert m.adapter_id is None and m.model._lora == [] and "LoRA" not in m.model.weights_source
    assert m.model.unet_config.time_cond_proj_dim == 256
    # with the key present the LoRA is loaded as before
    m2 = _method("consistency_model_config.yaml")
    assert m2.adapter_id == "latent-consistency/lcm-lora-sdv1-5" and len(m2.model._lora) == 1
    assert m2.model.unet_config.time_cond_proj_dim is None
