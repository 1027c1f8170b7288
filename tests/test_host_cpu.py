"""CPU: host-side logic of the product -- plugin surface, config entry points, C-ABI exports,
parameter enumeration, scheduler coefficient math (checked against the oracle's literal
restatement), batch sharding.  No compute call is made (no GPU here)."""
import ctypes as C
import math
import numpy as np
import os

import pytest
import torch

import sonicdiffusionbayeslab_amd as pkg
from sonicdiffusionbayeslab_amd import _lib
from sonicdiffusionbayeslab_amd.config import load_named_config
from sonicdiffusionbayeslab_amd.schedulers import DDIMSchedulerMy, DPMSolverScheduler, LCMScheduler, PNDMConfigStub
from sonicdiffusionbayeslab_amd.weights import UNetConfig, make_synthetic_state_dict, param_shapes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_registry_keys_match_reference_surface():
    # src/registry.py:3-6 + the decorator keys of the in-scope plugins
    assert set(pkg.methods_registry.keys()) >= {"ddim", "dpm_solver", "consistency_model", "deep_cache"}
    assert set(pkg.schedulers_registry.keys()) >= {"ddim_scheduler", "dpm_solver_scheduler", "lcm_scheduler"}
    assert "stable_diffusion_model" in pkg.models_registry
    assert {"time_metric", "clip_score"} <= set(pkg.metrics_registry.keys())
    assert pkg.schedulers_registry["dpm_solver_scheduler"] is DPMSolverScheduler
    # add_to_registry also records a dataclass of the __init__ signature (class_registry.py:58-68)
    assert "ddim_scheduler" in pkg.schedulers_registry.args


def test_class_registry_decorator():
    from sonicdiffusionbayeslab_amd.utils.class_registry import ClassRegistry
    r = ClassRegistry()

    @r.add_to_registry("thing")
    class Thing:
        def __init__(self, a, b=3, c=None, *args, **kwargs):
            pass

    assert r["thing"] is Thing
    f = {x.name: x for x in __import__("dataclasses").fields(r.args["thing"])}
    assert set(f) == {"a", "b", "c"} and f["b"].default == 3 and f["c"].default is None and f["a"].default == "???"
    with pytest.raises(KeyError):
        r["missing"]


@pytest.mark.parametrize("name,method", [("ddim_config.yaml", "ddim"), ("dpm_solver_config.yaml", "dpm_solver"),
                                         ("consistency_model_config.yaml", "consistency_model"),
                                         ("deep_cache_config.yaml", "deep_cache")])
def test_yaml_entry_points(name, method):
    cfg = load_named_config(name, os.path.join(ROOT, "configs"))
    assert cfg.experiment.method == method and cfg.experiment.get("seed", 29) == 29
    assert cfg.model.model_name == "stable_diffusion_model"
    assert method in pkg.methods_registry
    assert cfg.inference.get("batch_size", 1) == 32 and cfg.inference.get("nope", None) is None
    assert isinstance(cfg.experiment_params.num_inference_steps, list)
    with pytest.raises(AttributeError):
        cfg.experiment.missing_key
    assert os.path.exists(os.path.join(ROOT, cfg.dataset.prompts))


def test_prompt_dataset_order():
    from sonicdiffusionbayeslab_amd.dataset import PromptDataset
    ds = PromptDataset("./does/not/exist", os.path.join(ROOT, "data/dataset/img2annotations_test.json"))
    assert len(ds) == 1000
    b = next(ds.batches(32))
    assert len(b["prompt"]) == 32 and b["prompt"][0] == "a man on a snowboard is coming down a slope"
    assert sum(len(x["prompt"]) for x in ds.batches(32)) == 1000        # last batch is ragged (8)


def test_abi_library_exports_every_declared_symbol():
    lib = _lib.load()
    names = _lib.declared_symbols()
    assert len(names) >= 20
    for n in names:
        assert hasattr(lib, n), f"{n} declared in include/sd_hip.h but not exported"
    assert set(names) == set(_lib._SIGS), set(names) ^ set(_lib._SIGS)
    assert lib.sd_abi_version() == 3


def test_amax_operator_symbol_is_exported_and_the_abi_version_stays():
    """sd_op_amax_e4m3 (the measurement of sd_unet_calibrate_fp8 as an operator, tests/test_fp8_gpu.py) is additive."""
    lib = _lib.load()
    n = "sd_op_amax_e4m3"
    assert hasattr(lib, n), n
    assert n in _lib._SIGS and n in _lib.declared_symbols(), n
    assert lib.sd_abi_version() == 3


def test_param_enumeration_matches_library():
    from sonicdiffusionbayeslab_amd.unet import _c_config
    lib = _lib.load()
    cfg = UNetConfig()
    h = C.c_void_p()
    _lib.check(lib.sd_unet_create(C.byref(_c_config(cfg)), C.byref(h)))
    shapes = param_shapes(cfg)
    assert lib.sd_unet_num_params(h) == len(shapes) == 686
    assert sum(math.prod(s) for _, s in shapes) == 859520964          # SD-1.5 UNet: 859.5 M parameters
    name = C.create_string_buffer(256); shp = (C.c_longlong * 4)(); nd = C.c_int()
    for i, (n, s) in enumerate(shapes):
        _lib.check(lib.sd_unet_param_info(h, i, name, 256, shp, C.byref(nd)))
        assert name.value.decode() == n and tuple(shp[: nd.value]) == tuple(s), (i, n)
    # error behaviour: unknown parameter / wrong size / finalize with missing parameters
    buf = torch.zeros(4)
    assert lib.sd_unet_load_param(h, b"nope.weight", buf.data_ptr(), 4) != 0
    assert b"unknown parameter" in lib.sd_last_error()
    assert lib.sd_unet_load_param(h, b"conv_in.bias", buf.data_ptr(), 4) != 0
    assert lib.sd_unet_finalize(h) != 0 and b"never loaded" in lib.sd_last_error()
    lib.sd_unet_destroy(h)
    bad = UNetConfig(block_out_channels=(100, 200, 400, 400))
    assert lib.sd_unet_create(C.byref(_c_config(bad)), C.byref(h)) != 0


def test_vae_param_enumeration_matches_library():
    from sonicdiffusionbayeslab_amd.vae import VaeConfig, _c_config, vae_param_shapes
    lib = _lib.load()
    cfg = VaeConfig()
    h = C.c_void_p()
    _lib.check(lib.sd_vae_create(C.byref(_c_config(cfg)), C.byref(h)))
    shapes = vae_param_shapes(cfg)
    assert lib.sd_unet_num_params(h) == len(shapes) == 140
    assert sum(math.prod(s) for _, s in shapes) == 49490199          # SD-1.5 VAE decoder + post_quant_conv
    name = C.create_string_buffer(256); shp = (C.c_longlong * 4)(); nd = C.c_int()
    for i, (n, s) in enumerate(shapes):
        _lib.check(lib.sd_unet_param_info(h, i, name, 256, shp, C.byref(nd)))
        assert name.value.decode() == n and tuple(shp[: nd.value]) == tuple(s), (i, n)
    lib.sd_unet_destroy(h)


def test_product_fails_loudly_without_gpu():
    from sonicdiffusionbayeslab_amd.unet import HipUNet2DConditionModel
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(_lib.SdHipError):
        HipUNet2DConditionModel(UNetConfig(sample_size=8), {})
    s = DDIMSchedulerMy.from_config(PNDMConfigStub().config)
    s.set_timesteps(5)
    with pytest.raises(_lib.SdHipError):          # CPU tensors are refused, nothing falls back to torch
        s.step(torch.zeros(1, 4, 8, 8), 801, torch.zeros(1, 4, 8, 8))


def test_scheduler_from_config_inherits_checkpoint_settings():
    base = PNDMConfigStub().config
    d = DDIMSchedulerMy.from_config(base)
    assert d.config.steps_offset == 1 and d.config.set_alpha_to_one is False and d.config.timestep_spacing == "leading"
    p = DPMSolverScheduler.from_config(base, solver_order=2, algorithm_type="dpmsolver++", final_sigmas_type="zero")
    assert p.config.timestep_spacing == "leading" and p.config.solver_order == 2 and "skip_prk_steps" not in p.config
    with pytest.raises(ValueError):
        DPMSolverScheduler.from_config(base, algorithm_type="dpmsolver", final_sigmas_type="zero")
    l = LCMScheduler.from_config(base)
    l.set_timesteps(4)
    assert l._timesteps_list == [999, 759, 499, 259]
    with pytest.raises(NotImplementedError):
        PNDMConfigStub().set_timesteps(50)
    from sonicdiffusionbayeslab_amd.schedulers import PNDMScheduler
    pn = PNDMScheduler.from_config(base)
    pn.set_timesteps(50)
    assert pn._timesteps_list[:5] == [981, 961, 961, 941, 921] and len(pn._timesteps_list) == 51   # A.7


def test_ddim_host_coefficients_match_oracle():
    from oracle.schedulers import DDIMOracle
    s = DDIMSchedulerMy.from_config(PNDMConfigStub().config); s.set_timesteps(50)
    o = DDIMOracle(); o.set_timesteps(50)
    assert s._timesteps_list == [int(t) for t in o.timesteps]
    g = torch.Generator().manual_seed(0)
    x, e = torch.randn(64, generator=g), torch.randn(64, generator=g)
    for t in (981, 501, 21, 1):
        cx, ce, dx, de = s.coefficients(t)
        prev, x0 = o.step(e, t, x)
        assert torch.allclose(cx * x + ce * e, prev, rtol=2e-5, atol=2e-5)
        assert torch.allclose(dx * x + de * e, x0, rtol=2e-5, atol=2e-4)


@pytest.mark.parametrize("algo,order,fst,n", [("dpmsolver++", 2, "zero", 20), ("dpmsolver++", 3, "zero", 6),
                                               ("dpmsolver++", 1, "zero", 4), ("dpmsolver", 2, "sigma_min", 10),
                                               ("dpmsolver", 3, "sigma_min", 20), ("dpmsolver++", 2, "zero", 3),
                                               # SDE variants (src/schedulers.py:134-147)
                                               ("sde-dpmsolver++", 2, "zero", 20), ("sde-dpmsolver++", 1, "zero", 5),
                                               ("sde-dpmsolver++", 3, "zero", 25), ("sde-dpmsolver++", 2, "sigma_min", 8),
                                               ("sde-dpmsolver", 2, "sigma_min", 12), ("sde-dpmsolver", 1, "sigma_min", 6)])
def test_dpm_host_coefficients_match_oracle(algo, order, fst, n):
    """The fused kernel's scalar coefficients reproduce the oracle's literal multistep update when
    applied with torch on CPU (same linear combination the kernel evaluates)."""
    from oracle.schedulers import DPMSolverOracle
    base = PNDMConfigStub().config
    s = DPMSolverScheduler.from_config(base, solver_order=order, algorithm_type=algo, final_sigmas_type=fst)
    o = DPMSolverOracle(solver_order=order, algorithm_type=algo, final_sigmas_type=fst)
    s.set_timesteps(n); o.set_timesteps(n)
    assert s._timesteps_list == [int(t) for t in o.timesteps]
    assert torch.allclose(torch.from_numpy(s.sigmas), o.sigmas)
    g = torch.Generator().manual_seed(1)
    x = torch.randn(128, generator=g, dtype=torch.float64)
    hist, lower = [], 0
    for i, t in enumerate(s._timesteps_list):
        e = torch.randn(128, generator=g, dtype=torch.float64)
        z = torch.randn(128, generator=g, dtype=torch.float64)
        ref_prev, ref_x0 = o.step(e.float(), t, x.float(), variance_noise=z.float() if algo.startswith("sde") else None)
        lof = (i == n - 1) and ((n < 15) or fst == "zero")
        los = (i == n - 2) and n < 15
        k = 1 if (order == 1 or lower < 1 or lof) else (2 if (order == 2 or lower < 2 or los) else 3)
        yx, ye, mx, me = s._convert_coefs(i)
        px, pe, p1, p2, pn = s._update_coefs(i, k, mx, me)
        assert (pn != 0.0) == (algo.startswith("sde") and float(s.sigmas[i + 1]) > 0)
        prev = px * x + pe * e + (p1 * hist[-1] if k >= 2 else 0) + (p2 * hist[-2] if k >= 3 else 0) + pn * z
        assert torch.allclose(prev.float(), ref_prev, rtol=3e-4, atol=3e-4), (i, k)
        assert torch.allclose((yx * x + ye * e).float(), ref_x0, rtol=3e-4, atol=3e-3), i
        hist.append(mx * x + me * e)
        lower = min(lower + 1, order)
        x = ref_prev.double()


def test_pndm_host_coefficients_match_oracle():
    """PLMS weights and the prev-sample coefficients of the fused kernel vs the oracle's literal
    restatement of diffusers' PNDMScheduler.step_plms (applied with torch on the CPU)."""
    from oracle.schedulers import PNDMOracle
    from sonicdiffusionbayeslab_amd.schedulers import PNDMScheduler
    s = PNDMScheduler.from_config(PNDMConfigStub().config)
    o = PNDMOracle()
    s.set_timesteps(10); o.set_timesteps(10)
    assert s._timesteps_list == [int(t) for t in o.timesteps]
    g = torch.Generator().manual_seed(3)
    x = torch.randn(64, generator=g, dtype=torch.float64)
    hist, cur, ratio = [], None, 100
    W = {0: (1.0,), 1: (1.5, -0.5), 2: (23 / 12, -16 / 12, 5 / 12), 3: (55 / 24, -59 / 24, 37 / 24, -9 / 24)}
    for i, t in enumerate(s._timesteps_list):
        e = torch.randn(64, generator=g, dtype=torch.float64)
        (ref,) = o.step(e.float(), t, x.float())
        if i != 1:
            n = min(len(hist), 3)
            sc, k = s._prev_coefs(t, t - ratio)
            comb = W[n][0] * e + sum(W[n][j + 1] * hist[-1 - j] for j in range(n))
            prev = sc * x + k * comb
            hist = (hist + [e])[-4:]
            if i == 0:
                cur = x
        else:
            sc, k = s._prev_coefs(t + ratio, t)
            prev = sc * cur + k * 0.5 * (e + hist[-1])
        assert torch.allclose(prev.float(), ref, rtol=2e-5, atol=2e-5), i
        x = ref.double()


def test_shard_range_and_global_latents():
    from sonicdiffusionbayeslab_amd.dist import global_latents, shard_range
    for n, w in ((8, 1), (64, 4), (256, 8), (10, 4), (3, 8)):
        spans = [shard_range(n, r, w) for r in range(w)]
        assert spans[0][0] == 0 and spans[-1][1] == n
        assert all(a[1] == b[0] for a, b in zip(spans, spans[1:]))
        assert max(h - l for l, h in spans) - min(h - l for l, h in spans) <= 1
    a, b = global_latents(16, 4, 8, 29), global_latents(16, 4, 8, 29)
    assert torch.equal(a, b) and a.shape == (16, 4, 8, 8)
    with pytest.raises(ValueError):
        shard_range(4, 4, 4)


def test_synthetic_weights_are_seeded_and_on_bf16_grid():
    cfg = UNetConfig(sample_size=8, block_out_channels=(64, 128, 128, 128), num_heads=2, cross_attention_dim=64)
    a, b = make_synthetic_state_dict(cfg, 7), make_synthetic_state_dict(cfg, 7)
    assert a.keys() == b.keys() and all(torch.equal(a[k], b[k]) for k in a)
    w = a["down_blocks.0.resnets.0.conv1.weight"]
    assert torch.equal(w, w.to(torch.bfloat16).float())
    assert abs(float(a["conv_norm_out.weight"].mean()) - 1.0) < 0.1


# ---------------------------------------------------------------- variant pipelines, host logic
def test_variant_registry_keys():
    from sonicdiffusionbayeslab_amd.registry import methods_registry, models_registry
    for k in ("stable_diffusion_model_two_schedulers", "stable_diffusion_model_interliving_schedulers",
              "stable_diffusion_model_skip_timesteps"):
        assert models_registry[k] is not None
    for k in ("two_schedulers", "interliving_schedulers", "skip_steps"):
        assert methods_registry[k] is not None


def test_switch_timestamp_matches_oracle_and_reference_rules():
    """src/models.py:704-730 on the DDIM(10) schedule handed to DPM as custom timesteps."""
    from oracle.pipeline import switch_timestamp as o_switch
    from sonicdiffusionbayeslab_amd.models import StableDiffusionModelTwoSchedulers as M
    first = [901, 801, 701, 601, 501, 401, 301, 201, 101, 1]
    second = [950, 850, 710, 690, 500, 300, 100]
    for kind, want in (("closest", [710, 690, 500, 300, 100]),          # |710-701| = 9 is the minimum
                       ("left_closest", [710, 690, 500, 300, 100]),      # last entry >= 701
                       ("right_closest", [690, 500, 300, 100])):         # first entry <= 701
        f, s = M.switch_timestamp(first, second, 3, kind)
        assert f == [901, 801, 701] and s == want, (kind, s)
        assert (f, s) == o_switch(first, second, 3, kind)
    # identical schedules (what the pipeline really passes): the switch timestep is taken twice, once by each scheduler
    f, s = M.switch_timestamp(first, first, 4, "closest")
    assert f == first[:4] and s == first[3:]


def test_interleave_plan_matches_oracle():
    """src/models.py:952-966: groups of `solver_order` main steps -> one inter step at the group's first timestep."""
    from oracle.pipeline import interleave_plan as o_plan
    from sonicdiffusionbayeslab_amd.models import StableDiffusionModelInterlivingSchedulers as M
    ts = list(range(900, 0, -100))          # 9 steps
    keep, t_inter = M.interleave_plan(ts, 2, [1, 3])
    assert keep == [900, 800, 700, 500, 400, 300, 100] and t_inter == [700, 300]
    assert (keep, t_inter) == o_plan(ts, 2, [1, 3])
    keep, t_inter = M.interleave_plan(ts, 3, [0])
    assert keep == [900, 600, 500, 400, 300, 200, 100] and t_inter == [900]


def test_dpm_custom_timesteps_match_oracle():
    """set_timesteps(timesteps=...) (two-scheduler pipeline, src/models.py:488-492): same sigma table as the oracle."""
    import numpy as np
    from oracle.schedulers import DDIMOracle, DPMSolverOracle
    from sonicdiffusionbayeslab_amd.schedulers import DDIMSchedulerMy, DPMSolverScheduler, PNDMConfigStub
    kw = dict(solver_order=2, algorithm_type="dpmsolver++", final_sigmas_type="zero")
    d = DDIMSchedulerMy.from_config(PNDMConfigStub().config); d.set_timesteps(10)
    s = DPMSolverScheduler.from_config(PNDMConfigStub().config, **kw); s.set_timesteps(timesteps=d._timesteps_list)
    od = DDIMOracle(); od.set_timesteps(10)
    o = DPMSolverOracle(**kw); o.set_timesteps(timesteps=[int(t) for t in od.timesteps])
    assert s._timesteps_list == [int(t) for t in o.timesteps] == d._timesteps_list
    assert s.num_inference_steps == 10 and len(s.sigmas) == 11
    np.testing.assert_allclose(np.asarray(s.sigmas), o.sigmas.numpy(), rtol=1e-6)
    with pytest.raises(ValueError):
        s.set_timesteps()


def test_fuse_lora_state_dict_kohya_and_peft_layouts():
    """load_lora_weights + fuse_lora (src/experiments/consistency_model.py:20-21) on the host weights."""
    from sonicdiffusionbayeslab_amd.weights import fuse_lora_state_dict
    g = torch.Generator().manual_seed(3)
    r16 = lambda t: t.to(torch.bfloat16).float()
    lin, conv = "down_blocks.0.attentions.0.transformer_blocks.0.attn1.to_q", "down_blocks.0.resnets.0.conv1"
    base = {lin + ".weight": r16(torch.randn(64, 64, generator=g)), conv + ".weight": r16(torch.randn(64, 64, 3, 3, generator=g)),
            conv + ".bias": torch.zeros(64)}
    dl, ul = torch.randn(4, 64, generator=g), torch.randn(64, 4, generator=g)
    dc, uc = torch.randn(4, 64, 3, 3, generator=g), torch.randn(64, 4, 1, 1, generator=g)
    want_lin = r16(base[lin + ".weight"] + 0.5 * (8.0 / 4) * ul @ dl)
    want_conv = r16(base[conv + ".weight"] + 0.5 * (8.0 / 4) * torch.einsum("or,rikl->oikl", uc[:, :, 0, 0], dc))
    kohya = {"lora_unet_" + lin.replace(".", "_") + ".lora_down.weight": dl, "lora_unet_" + lin.replace(".", "_") + ".lora_up.weight": ul,
             "lora_unet_" + lin.replace(".", "_") + ".alpha": torch.tensor(8.0),
             "lora_unet_" + conv.replace(".", "_") + ".lora_down.weight": dc, "lora_unet_" + conv.replace(".", "_") + ".lora_up.weight": uc,
             "lora_unet_" + conv.replace(".", "_") + ".alpha": torch.tensor(8.0),
             "lora_te_text_model_encoder_layers_0_mlp_fc1.lora_down.weight": torch.zeros(4, 8)}
    sd = dict(base)
    assert fuse_lora_state_dict(sd, kohya, scale=0.5) == 2
    assert torch.equal(sd[lin + ".weight"], want_lin) and torch.equal(sd[conv + ".weight"], want_conv)
    peft = {"unet." + lin + ".lora_A.weight": dl, "unet." + lin + ".lora_B.weight": ul}          # alpha = r
    sd = dict(base)
    assert fuse_lora_state_dict(sd, peft, scale=1.0) == 1
    assert torch.equal(sd[lin + ".weight"], r16(base[lin + ".weight"] + ul @ dl))
    with pytest.raises(KeyError):
        fuse_lora_state_dict(dict(base), {"lora_unet_no_such_module.lora_down.weight": dl}, 1.0)


@pytest.mark.parametrize("dtype", ["bf16", "fp8"])
def test_finalize_packs_weights_on_the_host(dtype):
    """sd_unet_finalize repacks (and for fp8 quantises) on the host BEFORE it touches the device, so the packer runs
    here without a GPU: the e4m3 codes and per-output-channel scales it writes must equal the oracle's quantiser
    (oracle/fp8.py) bit for bit, in the layouts the kernels read."""
    from oracle.fp8 import quantize_rows
    from sonicdiffusionbayeslab_amd.unet import _c_config
    from sonicdiffusionbayeslab_amd.weights import make_synthetic_state_dict
    if torch.cuda.is_available():
        pytest.skip("host-side packer check runs on the CPU-only box (the blob is released after a successful upload)")
    lib = _lib.load()
    cfg = UNetConfig(sample_size=8, block_out_channels=(320, 640), attn_levels=(True, False))
    sd = make_synthetic_state_dict(cfg, seed=5)
    h = C.c_void_p()
    _lib.check(lib.sd_unet_create(C.byref(_c_config(cfg, dtype)), C.byref(h)))
    for name, shape in param_shapes(cfg):
        t = sd[name].float().contiguous()
        _lib.check(lib.sd_unet_load_param(h, name.encode(), t.data_ptr(), t.numel()))
    rc = lib.sd_unet_finalize(h)
    assert rc == -2 and b"hipMalloc" in lib.sd_last_error()           # packed, then no device to upload to

    def packed(key, nbytes, dt):
        buf = torch.empty(nbytes, dtype=torch.uint8)
        assert lib.sd_unet_debug_packed(h, key.encode(), buf.data_ptr(), nbytes) >= 0, lib.sd_last_error()
        return buf.view(dt)

    def same_codes(a, b):                                             # +0 and -0 are the same value
        return ((a == b) | (((a & 0x7f) == 0) & ((b & 0x7f) == 0))).all()

    p = "down_blocks.1.resnets.0."                                    # 320 -> 640 channels
    w = sd[p + "conv1.weight"]
    if dtype == "bf16":
        got = packed(p + "conv1.weight", w.numel() * 2, torch.bfloat16).view(640, 5, 9, 64)
        assert torch.equal(got.float(), w.permute(0, 2, 3, 1).reshape(640, 9, 5, 64).permute(0, 2, 1, 3).bfloat16().float())
        assert lib.sd_unet_debug_packed(h, (p + "conv1.weight.fp8").encode(), None, 0) < 0
        # ff.net.2 + proj_out merged into one two-segment-K GEMM: rows [bf16(Wpo W2) | bf16(Wpo)], bias Wpo b2 + bpo
        a = "down_blocks.0.attentions.0."
        t = a + "transformer_blocks.0."
        w2, b2 = sd[t + "ff.net.2.weight"].double(), sd[t + "ff.net.2.bias"].double()
        wpo, bpo = sd[a + "proj_out.weight"].double().view(320, 320), sd[a + "proj_out.bias"].double()
        got = packed(a + "ff_out.weight", 320 * 1600 * 2, torch.bfloat16).view(320, 1600).float()
        want = torch.cat([wpo @ w2, wpo], dim=1).float()
        assert (got - want).abs().max() <= 2.0 ** -8 * want.abs().max()                  # one bf16 rounding of an fp32 product
        assert torch.equal(got[:, 1280:], wpo.float().bfloat16().float())
        assert torch.allclose(packed(a + "ff_out.bias", 320 * 4, torch.float32), (wpo @ b2 + bpo).float(), rtol=1e-5, atol=1e-6)
        # upsampler as four 2x2 sub-pixel convs: [phase][O][I/64][tap][64], 3x3 taps that read the same low-res pixel summed
        wu = sd["up_blocks.0.upsamplers.0.conv.weight"].float()                       # [640, 640, 3, 3]
        rows = {0: ([0], [1, 2]), 1: ([0, 1], [2])}
        got = packed("up_blocks.0.upsamplers.0.conv.weight.sub", 4 * 640 * 640 * 4 * 2, torch.bfloat16).view(4, 640, 10, 4, 64)
        for py in (0, 1):
            for px in (0, 1):
                for dy in (0, 1):
                    for dx in (0, 1):
                        want = wu[:, :, rows[py][dy]][:, :, :, rows[px][dx]].sum((2, 3)).bfloat16()      # [O, I]
                        assert torch.equal(got[py * 2 + px, :, :, dy * 2 + dx, :].reshape(640, 640), want)
        # LayerNorm folded into q|k|v: rows bf16(W gamma), c1 = sum of the ROUNDED row, c2 = W beta; the W_q rows carry the
        # softmax scale and the exp -> exp2 factor, log2(e) / sqrt(head_dim), multiplied in fp32 before the rounding
        g1, be1 = sd[t + "norm1.weight"].float(), sd[t + "norm1.bias"].double()
        rows = torch.cat([sd[t + f"attn1.to_{x}.weight"] for x in "qkv"]).float()
        rows[:320] *= (torch.tensor(1.4426950408889634, dtype=torch.float32) / torch.sqrt(torch.tensor(40.0, dtype=torch.float32)))
        got = packed(t + "attn1.qkv.weight.ln", 960 * 320 * 2, torch.bfloat16).view(960, 320)
        assert torch.equal(got, (rows * g1[None, :]).bfloat16())
        assert torch.allclose(packed(t + "attn1.qkv.weight.c1", 960 * 4, torch.float32), got.double().sum(1).float(), rtol=1e-6, atol=1e-6)
        assert torch.allclose(packed(t + "attn1.qkv.weight.c2", 960 * 4, torch.float32), (rows.double() @ be1).float(), rtol=1e-5, atol=1e-6)
    else:
        q, scale = quantize_rows(w)
        codes = q.to(torch.float8_e4m3fn).view(torch.uint8)          # [640, 320, 3, 3]
        want = torch.zeros(640, 384, 3, 3, dtype=torch.uint8)        # Cin 320 padded to 3 slices of 128
        want[:, :320] = codes
        want = want.permute(0, 2, 3, 1).reshape(640, 9, 3, 128).permute(0, 2, 1, 3).contiguous()
        got = packed(p + "conv1.weight.fp8", 640 * 9 * 384, torch.uint8).view(640, 3, 9, 128)
        assert same_codes(got, want)
        assert torch.equal(packed(p + "conv1.weight.scale", 640 * 4, torch.float32), scale)
        # GEGLU rows: interleaved [16 value | 16 gate] per 32, K = 320 padded to 384
        t = "down_blocks.0.attentions.0.transformer_blocks.0."
        wq, sc = quantize_rows(sd[t + "ff.net.0.proj.weight"])       # [2560, 320]
        H = 1280
        idx = [g * 16 + k if k < 16 else H + g * 16 + k - 16 for g in range(2 * H // 32) for k in range(32)]
        got = packed(t + "ff.geglu.weight.fp8", 2 * H * 384, torch.uint8).view(2 * H, 384)
        want = wq[idx].to(torch.float8_e4m3fn).view(torch.uint8)
        assert same_codes(got[:, :320], want) and (got[:, 320:] == 0).all()
        assert torch.equal(packed(t + "ff.geglu.weight.scale", 2 * H * 4, torch.float32), sc[idx])
        # fused QKV rows of the self-attention
        rows = torch.cat([sd[t + f"attn1.to_{x}.weight"] for x in "qkv"]).float()
        rows[:320] *= (torch.tensor(1.4426950408889634, dtype=torch.float32) / torch.sqrt(torch.tensor(40.0, dtype=torch.float32)))    # W_q carries scale * log2 e
        wq, sc = quantize_rows(rows)
        got = packed(t + "attn1.qkv.weight.fp8", 960 * 384, torch.uint8).view(960, 384)
        assert same_codes(got[:, :320], wq.to(torch.float8_e4m3fn).view(torch.uint8)) and (got[:, 320:] == 0).all()
    lib.sd_unet_destroy(h)


def _host_pack_case(kind):
    """(create(handle) -> rc, parameter shapes, state dict) of the smallest config the GPU tests of `kind` use."""
    from sonicdiffusionbayeslab_amd import clip, clip_score, vae
    from tests.clip_score_util import tiny_configs, tiny_state_dict
    lib = _lib.load()
    if kind.startswith("vae"):
        cfg = vae.VaeConfig(sample_size=16)
        create, shapes = ((lib.sd_vae_create, vae.vae_param_shapes) if kind == "vae_decoder" else
                          (lib.sd_vae_encoder_create, vae.vae_encoder_param_shapes))
        c = vae._c_config(cfg)
        return (lambda h: create(C.byref(c), C.byref(h))), shapes(cfg), vae.make_synthetic_vae_state_dict(cfg)
    tcfg, vcfg = tiny_configs()
    if kind == "clip_text":
        c = _lib.SdClipConfig(tcfg.vocab_size, tcfg.hidden_size, tcfg.num_hidden_layers, tcfg.num_attention_heads,
                              tcfg.intermediate_size, tcfg.max_position_embeddings, tcfg.layer_norm_eps)
        return (lambda h: lib.sd_clip_create(C.byref(c), C.byref(h))), clip.clip_param_shapes(tcfg), tiny_state_dict()
    c = _lib.SdClipVisionConfig(vcfg.hidden_size, vcfg.num_hidden_layers, vcfg.num_attention_heads, vcfg.intermediate_size,
                                vcfg.image_size, vcfg.patch_size, vcfg.projection_dim, vcfg.layer_norm_eps)
    return (lambda h: lib.sd_clip_vision_create(C.byref(c), C.byref(h))), clip_score.clip_vision_param_shapes(vcfg), tiny_state_dict()


@pytest.mark.parametrize("kind,plain", [("vae_decoder", "decoder.conv_norm_out.weight"), ("vae_encoder", "encoder.conv_norm_out.weight"),
                                        ("clip_text", "text_model.final_layer_norm.weight"),
                                        ("clip_vision", "vision_model.post_layernorm.weight")])
def test_finalize_packs_the_other_handle_kinds_on_the_host(kind, plain):
    """The packers of the VAE decoder / encoder and of the two CLIP towers run here as the UNet's does above: finalize packs
    on the host and stops at the upload, and an fp32 vector the packer stores as the parameter itself (Packer::f32, under
    the parameter's own name) reads back bit-equal from the staging blob."""
    if torch.cuda.is_available():
        pytest.skip("host-side packer check runs on the CPU-only box (the blob is released after a successful upload)")
    lib = _lib.load()
    create, shapes, sd = _host_pack_case(kind)
    h = C.c_void_p()
    _lib.check(create(h))
    for name, shape in shapes:
        t = sd[name].float().contiguous()
        assert tuple(t.shape) == tuple(shape), name
        _lib.check(lib.sd_unet_load_param(h, name.encode(), t.data_ptr(), t.numel()))
    assert lib.sd_unet_finalize(h) == -2 and b"hipMalloc" in lib.sd_last_error()      # packed, then no device to upload to
    want = sd[plain].float().contiguous()
    got = torch.empty_like(want)
    assert lib.sd_unet_debug_packed(h, plain.encode(), got.data_ptr(), want.numel() * 4) >= 0, lib.sd_last_error()
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    lib.sd_unet_destroy(h)


def test_geglu_polynomial_gelu_error_bound():
    """The GEGLU epilogue's transcendental-free GELU (csrc/common.h::geglu_pair): its constants, evaluated in float32 the
    way the kernel does, stay within 1.3e-5 |x| of the exact-erf GELU (diffusers GEGLU -> F.gelu, approximate='none')."""
    import re
    from scipy.special import erf
    src = open(os.path.join(os.path.dirname(__file__), "..", "sonicdiffusionbayeslab_amd", "csrc", "common.h")).read()
    body = src[src.index("f32x2_t geglu_pair("):]
    body = body[:body.index("return value * gate * phi")]
    c = float(re.search(r"constexpr float C = ([0-9.]+)f", body).group(1))
    ks = [float(v) for v in re.findall(r"k\((-?[0-9.]+e[+-][0-9]+)f\)", body)]
    assert len(ks) == 10                                 # Horner order: highest power first
    x = np.linspace(-12, 12, 480001).astype(np.float32)
    xc = np.clip(x, -c, c).astype(np.float32)
    u = (xc * np.float32(1.0 / c)) ** 2
    p = np.full_like(u, np.float32(ks[0]))
    for k in ks[1:]:
        p = p * u + np.float32(k)
    got = x * (np.float32(0.5) + xc * p)
    x64 = x.astype(np.float64)
    ref = x64 * 0.5 * (1 + erf(x64 / np.sqrt(2)))
    assert (np.abs(got - ref) / np.maximum(np.abs(x64), 1e-3)).max() < 1.3e-5


# ---------------------------------------------------------------------------------------------------
# the path REAL weights take: from_pretrained(<local diffusers dir>) -> load_unet_config / load_unet_state_dict -> handle
# ---------------------------------------------------------------------------------------------------
def _write_tiny_diffusers_dir(root, cfg, sd, dtype=torch.float16):
    import json
    from safetensors.torch import save_file
    os.makedirs(os.path.join(root, "unet"), exist_ok=True)
    nl = len(cfg.block_out_channels)
    json.dump({"_class_name": "UNet2DConditionModel", "sample_size": cfg.sample_size, "in_channels": 4, "out_channels": 4,
               "block_out_channels": list(cfg.block_out_channels), "layers_per_block": cfg.layers_per_block,
               "down_block_types": ["CrossAttnDownBlock2D" if a else "DownBlock2D" for a in cfg.attn_levels],
               "up_block_types": ["CrossAttnUpBlock2D" if a else "UpBlock2D" for a in reversed(cfg.attn_levels)],
               "cross_attention_dim": cfg.cross_attention_dim, "attention_head_dim": cfg.num_heads, "norm_num_groups": 32,
               "norm_eps": 1e-5, "act_fn": "silu", "use_linear_projection": False, "flip_sin_to_cos": True, "freq_shift": 0},
              open(os.path.join(root, "unet", "config.json"), "w"))
    save_file({k: v.to(dtype) for k, v in sd.items()}, os.path.join(root, "unet", "diffusion_pytorch_model.safetensors"))
    assert nl == len(cfg.attn_levels)


def test_from_pretrained_local_directory_reaches_the_library(tmp_path):
    """``from_pretrained(<local dir>)`` (src/experiments/base_experiment.py:55-64): ``unet/config.json`` becomes the
    UNetConfig, the fp16 safetensors become the state dict, and every parameter the library enumerates for that config is
    accepted by ``sd_unet_load_param`` and packed by ``sd_unet_finalize`` (which then stops at the upload: no GPU here)."""
    from sonicdiffusionbayeslab_amd.models import StableDiffusionModel
    from sonicdiffusionbayeslab_amd.unet import _c_config, load_params
    from sonicdiffusionbayeslab_amd.weights import make_synthetic_state_dict
    cfg = UNetConfig(sample_size=8, block_out_channels=(320, 640), attn_levels=(True, False))
    sd = make_synthetic_state_dict(cfg, seed=11)
    _write_tiny_diffusers_dir(str(tmp_path), cfg, sd)
    m = StableDiffusionModel.from_pretrained(str(tmp_path), timestamps=None, safety_checker=None,
                                             requires_safety_checker=False, torch_dtype=torch.float16)
    assert m.weights_source == f"local:{tmp_path}" and m._clip_dir is None
    assert m.unet_config == cfg
    got = m._state_dict
    assert set(got) == {n for n, _ in param_shapes(cfg)}
    # bf16-grid values survive the fp16 file exactly only where fp16 can hold them; everything is within fp16 rounding
    for n, shape in param_shapes(cfg):
        assert tuple(got[n].shape) == tuple(shape) and got[n].dtype == torch.float32
        assert torch.allclose(got[n], sd[n], rtol=2 ** -10, atol=2 ** -24)
    lib = _lib.load()
    h = C.c_void_p()
    _lib.check(lib.sd_unet_create(C.byref(_c_config(m.unet_config)), C.byref(h)))
    load_params(lib, h, m.unet_config, got)
    if not torch.cuda.is_available():
        assert lib.sd_unet_finalize(h) == -2 and b"hipMalloc" in lib.sd_last_error()     # packed; no device to upload to
        assert lib.sd_unet_debug_packed(h, b"down_blocks.0.attentions.0.ff_out.weight", None, 0) >= 0
    lib.sd_unet_destroy(h)
    # a missing / mis-shaped parameter and an unsupported architecture key are refused, not mis-run
    bad = dict(got); bad.pop("conv_in.bias")
    h2 = C.c_void_p()
    _lib.check(lib.sd_unet_create(C.byref(_c_config(cfg)), C.byref(h2)))
    with pytest.raises(KeyError):
        load_params(lib, h2, cfg, bad)
    bad["conv_in.bias"] = torch.zeros(7)
    with pytest.raises(ValueError):
        load_params(lib, h2, cfg, bad)
    lib.sd_unet_destroy(h2)
    import json
    cj = os.path.join(str(tmp_path), "unet", "config.json")
    c = json.load(open(cj)); c["use_linear_projection"] = True; json.dump(c, open(cj, "w"))
    with pytest.raises(NotImplementedError):
        StableDiffusionModel.from_pretrained(str(tmp_path))
    # a hub NAME is never fetched: synthetic weights, and the report says so
    m2 = StableDiffusionModel.from_pretrained("runwayml/stable-diffusion-v1-5")
    assert m2.weights_source.startswith("synthetic(") and m2._state_dict is None


def _write_tiny_clip_dir(root):
    """A randomly initialised CLIP (text + vision towers, projection) with a synthetic byte-level BPE vocabulary, saved the
    way a local ``openai/clip-vit-base-patch16`` directory looks to ``CLIPModel / CLIPProcessor.from_pretrained``."""
    import json
    tr = pytest.importorskip("transformers")
    from tests.util import synthetic_clip_vocab
    vocab, merges = synthetic_clip_vocab()
    json.dump(vocab, open(os.path.join(root, "vocab.json"), "w"))
    open(os.path.join(root, "merges.txt"), "w").write("#version: 0.2\n" + "\n".join(f"{a} {b}" for a, b in merges) + "\n")
    tok = tr.CLIPTokenizer(os.path.join(root, "vocab.json"), os.path.join(root, "merges.txt"), model_max_length=16)
    ip = tr.CLIPImageProcessor(size={"shortest_edge": 32}, crop_size={"height": 32, "width": 32})
    tr.CLIPProcessor(image_processor=ip, tokenizer=tok).save_pretrained(root)
    eos = vocab["<|endoftext|>"]
    cfg = tr.CLIPConfig(text_config=dict(vocab_size=len(vocab), hidden_size=32, num_hidden_layers=1, num_attention_heads=2,
                                         intermediate_size=64, max_position_embeddings=16,
                                         bos_token_id=vocab["<|startoftext|>"], eos_token_id=eos, pad_token_id=eos),
                        vision_config=dict(hidden_size=32, num_hidden_layers=1, num_attention_heads=2, intermediate_size=64,
                                           image_size=32, patch_size=8), projection_dim=16)
    torch.manual_seed(0)
    tr.CLIPModel(cfg).eval().save_pretrained(root)


def test_clip_score_metric_and_its_wiring_into_validate(tmp_path, capsys):
    """``clip_score`` = mean over pairs of max(100 cos(E_img, E_txt), 0) (torchmetrics CLIPScore, SURVEY A.8;
    calc_clip_score.py:13-37) on a tiny random CLIP, and the harness: ``quality_metrics.clip_score.model_name_or_path``
    pointing at a local directory makes ``validate`` report it for decoded images (base_experiment.py:96-98,198-201)."""
    import json
    tr = pytest.importorskip("transformers")
    from sonicdiffusionbayeslab_amd.config import _wrap
    from sonicdiffusionbayeslab_amd.experiments.base_experiment import BaseMethod
    from sonicdiffusionbayeslab_amd.registry import metrics_registry
    root = str(tmp_path)
    _write_tiny_clip_dir(root)
    with pytest.raises(FileNotFoundError):
        metrics_registry["clip_score"]("openai/clip-vit-base-patch16")         # a hub name is never fetched
    metric = metrics_registry["clip_score"](root)
    g = torch.Generator().manual_seed(3)
    imgs = torch.rand((5, 3, 48, 40), generator=g)
    texts = ["A photo of the cat", "the hat", "", "photo of a thing", "x" * 100]
    u8 = (imgs * 255).to(torch.uint8)
    metric.update(u8[:3], texts[:3]); metric.update(u8[3:], texts[3:])
    model, proc = tr.CLIPModel.from_pretrained(root).eval(), tr.CLIPProcessor.from_pretrained(root)
    with torch.no_grad():
        inp = proc(text=texts, images=[i for i in u8], return_tensors="pt", padding=True, truncation=True)
        out = model(**inp)
    want = (100 * torch.nn.functional.cosine_similarity(out.image_embeds, out.text_embeds)).clamp(min=0).mean()
    assert abs(float(metric.compute()) - float(want)) < 1e-3

    class _Stub:
        weights_source, num_timesteps = "stub", 2

        def __init__(self):
            self.unet_config = UNetConfig(sample_size=8)
            self.scheduler = type("S", (), {"config": {}})()

        def to(self, device):
            return self

        def __call__(self, prompts, generator=None, output_type="pt", **kw):
            n = len(prompts)
            return type("O", (), {"images": torch.rand((n, 3, 64, 64), generator=generator)})(), 0.1, []

    class M(BaseMethod):
        def setup_model(self):
            self.model = _Stub()

        def setup_scheduler(self, **kw):
            pass

        def run_experiment(self):
            self.sweep([2], lambda n: {"num_inference_steps": n}, lambda n: f"steps {n}")

    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    base = {"experiment_name": "stub", "experiment": {"method": "stub", "seed": 29},
            "dataset": {"img_dataset": "", "prompts": os.path.join(repo, "data", "dataset", "img2annotations_test.json")},
            "inference": {"batch_size": 3, "batch_count": 2}}
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "SD_DIST_FORCE_INIT"):
        os.environ.pop(k, None)
    m = M(_wrap(dict(base, quality_metrics={"clip_score": {"model_name_or_path": root}})))
    m.device = "cpu"
    m.run_experiment()
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert line["images"] == 6 and line["clip_score_model"] == root and 0.0 <= line["clip_score"] <= 100.0
    assert m.metric_dict["clip_score"] == [line["clip_score"]]
    m2 = M(_wrap(dict(base, quality_metrics={"clip_score": {"model_name_or_path": "openai/clip-vit-base-patch16"}})))
    m2.device = "cpu"
    m2.run_experiment()
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert line["clip_score"] is None and "not computable offline" in line["clip_score_model"]


def test_postprocess_images_np_and_pil():
    """``output_type`` "np" / "pil" (``src/models.py:312-321``): diffusers' VaeImageProcessor.postprocess on images already
    denormalised to [0, 1] -- NHWC float32 on the host, or uint8 PIL images rounded from 255 x."""
    from sonicdiffusionbayeslab_amd.models import postprocess_images
    g = torch.Generator().manual_seed(4)
    img = torch.rand(2, 3, 8, 6, generator=g)
    assert postprocess_images(img, "pt") is img
    arr = postprocess_images(img, "np")
    assert arr.shape == (2, 8, 6, 3) and arr.dtype == np.float32
    assert np.array_equal(arr, img.permute(0, 2, 3, 1).numpy())
    pil = postprocess_images(img, "pil")
    assert len(pil) == 2 and pil[0].size == (6, 8) and pil[0].mode == "RGB"
    assert np.array_equal(np.asarray(pil[1]), (arr[1] * 255.0).round().astype(np.uint8))
    with pytest.raises(NotImplementedError):
        postprocess_images(img, "jpeg")


def test_model_registry_entries_are_the_pipeline_classes():
    """``models_registry[name].from_pretrained(...)`` is how the harness builds its model (``src/experiments/base_experiment.py:55-66``):
    every name the reference registers (``src/models.py:21,340,628,1048``) maps to a class with that constructor."""
    from sonicdiffusionbayeslab_amd import models
    from sonicdiffusionbayeslab_amd.registry import models_registry
    want = {"stable_diffusion_model": models.StableDiffusionModel,
            "stable_diffusion_model_two_schedulers": models.StableDiffusionModelTwoSchedulers,
            "stable_diffusion_model_interliving_schedulers": models.StableDiffusionModelInterlivingSchedulers,
            "stable_diffusion_model_skip_timesteps": models.StableDiffusionModelSkipTimesteps}
    for name, cls in want.items():
        assert models_registry[name] is cls and isinstance(cls, type) and callable(getattr(cls, "from_pretrained"))


def _library_asm():
    """lib/<unit>.s of every translation unit, left behind by the build that produced the objects (build.py, -save-temps).
    Skips when the build cannot be (re)done here; rebuilds when a source is newer than its assembly."""
    import os
    import shutil
    from sonicdiffusionbayeslab_amd import build as B
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    have_hipcc = os.path.exists(hipcc) or shutil.which("hipcc") is not None
    inputs = [os.path.normpath(os.path.join(B.CSRC, h)) for h in B.HEADERS]
    stale = [src for src in B.SOURCES if B._newer(os.path.join(B.CSRC, src), B.asm_path(src)) or any(B._newer(h, B.asm_path(src)) for h in inputs)]
    if stale:
        if not have_hipcc:
            pytest.skip(f"no hipcc here and the assembly of {stale} is missing or older than its source")
        B.build_library(verbose=False)
    return {src.split(".")[0]: B.asm_path(src) for src in B.SOURCES}


def test_library_assembly_passes_the_hazard_lint_and_the_lint_catches_mutations():
    """sonicdiffusionbayeslab_amd/asm_lint.py on the assembly of the objects in the tree (the build fails on a violation; this
    re-checks what is there) and, for every rule, a mutation of real assembly that the rule must catch:
    PK_OPSEL (the v_pk_fma_f32 op_sel form MI355X mis-executes beside MFMAs: round 4's LayerNorm-fold wrong result),
    STORE_SOFF (16-byte buffer store with an SGPR soffset: round 4, hazard 1), MFMA_DIST (a VALU read of an MFMA result
    before the hardware's measured minimum), LDS_WAITS (csrc/attention.hip's hand-counted lgkmcnt: a wait one too lax, a
    copy of a fragment register ahead of its wait)."""
    import re
    from sonicdiffusionbayeslab_amd import asm_lint as L
    paths = _library_asm()
    for unit, path in paths.items():
        assert L.lint_file(path, unit, verbose=False) == [], (unit, L.lint_file(path, unit, verbose=False)[:3])
    # ---- LDS_WAITS on the 64x64 self-attention kernel
    text = open(paths["attention"]).read()
    kernels = list(L.kernels(text, "attn_pipe40_kernelILi7"))
    assert len(kernels) == 1
    name, body = kernels[0]
    errs, n_tr = L.check_lds_waits(name, body)
    assert n_tr >= 32 and errs == [], errs[:3]
    lax = body.replace("s_waitcnt lgkmcnt(6)", "s_waitcnt lgkmcnt(7)", 1)
    assert lax != body and L.check_lds_waits(name, lax)[0]
    m = re.search(r"ds_read_b64_tr_b16 (v\[(\d+):\d+\]),[^\n]*\n", body)
    early = body[:m.end()] + f"\tv_mov_b32_e32 v255, v{m.group(2)}\n" + body[m.end():]
    assert L.check_lds_waits(name, early)[0]
    # ---- PK_OPSEL / STORE_SOFF / MFMA_DIST on the LayerNorm-fold GEMM
    name, body = next(L.kernels(open(paths["gemm_lean"]).read(), "gemm_lean_kernelILi128ELi160ELi2ELi2ELi4E"))
    assert L.check_pk_opsel(name, body) == [] and L.check_store_soffset(name, body) == [] and L.check_mfma_distance(name, body) == []
    m = re.search(r"\tv_fma_f32 (v\d+), (v\d+), (v\d+), (v\d+)\n", body)
    packed = body[:m.start()] + "\tv_pk_fma_f32 v[0:1], v[2:3], v[4:5], v[6:7] op_sel:[0,1,0]\n" + body[m.start():]
    assert len(L.check_pk_opsel(name, packed)) == 1
    ok_form = body[:m.start()] + "\tv_pk_fma_f32 v[0:1], v[2:3], v[4:5], v[6:7] op_sel_hi:[1,0,1] neg_lo:[0,1,0]\n" + body[m.start():]
    assert L.check_pk_opsel(name, ok_form) == []                      # (the hi-lane selection never failed on the hardware)
    m = re.search(r"buffer_store_dwordx4 (v\[\d+:\d+\]), (v\d+), (s\[\d+:\d+\]), 0 offen", body)
    soff = body.replace(m.group(0), f"buffer_store_dwordx4 {m.group(1)}, {m.group(2)}, {m.group(3)}, s31 offen", 1)
    assert len(L.check_store_soffset(name, soff)) == 1
    mf = list(re.finditer(r"\tv_mfma_f32_16x16x32_bf16 v\[(\d+):\d+\],[^\n]*\n", body))[-1]
    early_read = body[:mf.end()] + f"\ts_nop 5\n\tv_add_f32_e32 v255, 1.0, v{mf.group(1)}\n" + body[mf.end():]      # 6 wait states < 8
    assert any("MFMA_DIST" in e for e in L.check_mfma_distance(name, early_read))
    fine_read = body[:mf.end()] + f"\ts_nop 7\n\tv_add_f32_e32 v255, 1.0, v{mf.group(1)}\n" + body[mf.end():]       # hipcc's own padding
    assert L.check_mfma_distance(name, fine_read) == []
