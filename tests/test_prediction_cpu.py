"""v-prediction / sample prediction, zero-terminal-SNR schedules and the checkpoint's scheduler config, without a GPU.

The host coefficient tests run the schedulers' real ``step_fused`` with the fused launch replaced by a float64 CPU
evaluation of the kernel's documented formula (include/sd_hip.h: sd_sched_step / sd_sched_step_rescaled), and compare
every step of full schedules with the fp64 restatement in tests/sched_ref.py."""
import json
import os

import numpy as np
import pytest
import torch

from sonicdiffusionbayeslab_amd import schedulers as S
from sonicdiffusionbayeslab_amd.schedulers import (DDIMSchedulerMy, DPMSolverScheduler, LCMScheduler, PNDMConfigStub,
                                                   PNDMScheduler, SD15_SCHEDULER_CONFIG)
from tests import sched_ref as R


# ------------------------------------------------------------------------------------------------ zero-SNR tables
@pytest.mark.parametrize("cls", [DDIMSchedulerMy, LCMScheduler, DPMSolverScheduler])
def test_zero_snr_tables(cls):
    base = PNDMConfigStub().config
    plain = cls.from_config(base).alphas_cumprod
    s = cls.from_config(base, rescale_betas_zero_snr=True, prediction_type="v_prediction")
    ac = s.alphas_cumprod
    assert ac.dtype == np.float32
    assert ac[0] == plain[0]                       # the first alpha_bar is kept
    if cls is DPMSolverScheduler:
        assert ac[-1] == np.float32(2.0 ** -24)     # upstream: close to 0, so that the first sigma is finite
    else:
        assert ac[-1] == 0.0
    betas = R.betas_fp32()
    ref = R.alphas_cumprod(betas, zero_snr=True)
    got = torch.from_numpy(ac).double()
    n = 999 if cls is DPMSolverScheduler else 1000
    ratio = ((got[:n] - ref[:n]).abs() / R.zero_snr_table_bound(betas)[:n]).max().item()
    print(f"{cls.__name__}: zero-SNR table worst error / bound {ratio:.3e}")
    assert ratio <= 1.0
    assert (np.diff(ac[:n]) < 0).all()             # still strictly decreasing


def test_zero_snr_key_propagation():
    ckpt = dict(SD15_SCHEDULER_CONFIG, _class_name="DDIMScheduler", prediction_type="v_prediction",
                rescale_betas_zero_snr=True, timestep_spacing="trailing")
    for cls in (DDIMSchedulerMy, DPMSolverScheduler, LCMScheduler):
        s = cls.from_config(ckpt)
        assert s.config.prediction_type == "v_prediction" and s.config.rescale_betas_zero_snr is True
        assert "_class_name" not in s.config
    p = PNDMScheduler.from_config(ckpt, timestep_spacing="leading")       # PNDM does not take the key: dropped, as upstream
    assert "rescale_betas_zero_snr" not in p.config and p.config.prediction_type == "v_prediction"
    assert p.alphas_cumprod[-1] > 0
    with pytest.raises(ValueError, match="prediction_type"):
        PNDMScheduler.from_config(ckpt, prediction_type="sample", timestep_spacing="leading")
    for cls in (DDIMSchedulerMy, DPMSolverScheduler, LCMScheduler):  # unchanged refusals
        with pytest.raises(NotImplementedError):
            cls.from_config(ckpt, prediction_type="flow_prediction")
        with pytest.raises(NotImplementedError):
            cls.from_config(ckpt, thresholding=True)


def test_epsilon_at_zero_snr_is_refused_at_set_timesteps():
    base = PNDMConfigStub().config
    d = DDIMSchedulerMy.from_config(base, rescale_betas_zero_snr=True, timestep_spacing="trailing")
    with pytest.raises(ValueError, match="epsilon.*rescale_betas_zero_snr.*trailing"):
        d.set_timesteps(10)
    DDIMSchedulerMy.from_config(base, rescale_betas_zero_snr=True).set_timesteps(50)   # "leading": never reaches t = 999
    with pytest.raises(ValueError, match="epsilon"):
        LCMScheduler.from_config(base, rescale_betas_zero_snr=True).set_timesteps(4)
    DPMSolverScheduler.from_config(base, rescale_betas_zero_snr=True, timestep_spacing="trailing").set_timesteps(10)
    DDIMSchedulerMy.from_config(base, rescale_betas_zero_snr=True, timestep_spacing="trailing",
                                prediction_type="v_prediction").set_timesteps(10)


# ------------------------------------------------------------------------------------------------ host coefficients
def _cpu_launch(eps, cfg, guidance, x, m1, m2, noise, coef, want_y2=True, want_m=False, m3=None, k=None):
    """The kernel's formula (include/sd_hip.h) in float64 on the CPU."""
    c = [float(v) for v in coef] + [0.0] * (10 - len(coef))
    B = x.shape[0]
    e = eps[:B] + guidance * (eps[B:] - eps[:B]) if cfg else eps
    if k is not None:
        e = e * k.view(-1, *([1] * (e.dim() - 1)))
    prev = c[0] * x + c[1] * e
    for w, m in ((c[2], m1), (c[3], m2), (c[9], m3), (c[4], noise)):
        if m is not None:
            prev = prev + w * m
    return prev, (c[5] * x + c[6] * e) if want_y2 else None, (c[7] * x + c[8] * e) if want_m else None


def _cpu_factors(eps, batch, guidance, rescale):
    u, c = eps.double().chunk(2)
    return R.rescale_factor(R.cfg_combine(u, c, guidance), c, rescale).flatten()


@pytest.fixture
def cpu_step(monkeypatch):
    monkeypatch.setattr(S._FusedStepScheduler, "_launch", staticmethod(_cpu_launch))
    monkeypatch.setattr(S._FusedStepScheduler, "_prep", staticmethod(lambda t: t.double()))
    monkeypatch.setattr(S, "cfg_rescale_factors", _cpu_factors)


CASES = [("ddim", {"timestep_spacing": "trailing"}, 12), ("ddim", {}, 10),
         ("lcm", {}, 4),
         ("pndm", {}, 8),
         ("dpm", dict(solver_order=1, algorithm_type="dpmsolver++", timestep_spacing="trailing"), 6),
         ("dpm", dict(solver_order=2, algorithm_type="dpmsolver++", timestep_spacing="trailing"), 20),
         ("dpm", dict(solver_order=3, algorithm_type="dpmsolver++", timestep_spacing="trailing"), 20),
         ("dpm", dict(solver_order=2, algorithm_type="dpmsolver", final_sigmas_type="sigma_min"), 12),
         ("dpm", dict(solver_order=3, algorithm_type="dpmsolver", final_sigmas_type="sigma_min"), 20),
         ("dpm", dict(solver_order=2, algorithm_type="sde-dpmsolver++", timestep_spacing="trailing"), 10),
         ("dpm", dict(solver_order=3, algorithm_type="sde-dpmsolver++", timestep_spacing="trailing"), 20),
         ("dpm", dict(solver_order=2, algorithm_type="sde-dpmsolver", final_sigmas_type="sigma_min"), 8)]


def _ids(c):
    return f"{c[0]}-{'-'.join(f'{v}' for v in c[1].values())}-{c[2]}"


def _runs(case, pred, zero_snr):
    kind, kw, _ = case
    if kind == "pndm" and pred == "sample":
        return False                # PNDM takes epsilon and v_prediction only (refusal tested above)
    if kind in ("ddim", "lcm") and pred == "epsilon" and zero_snr and (kind == "lcm" or "timestep_spacing" in kw):
        return False                # refused at set_timesteps (tested above)
    return True


GRID = [(c, p, z) for c in CASES for p in ("epsilon", "v_prediction", "sample") for z in (False, True) if _runs(c, p, z)]


@pytest.mark.parametrize("case,pred,zero_snr", GRID, ids=[f"{_ids(c)}-{p}-{'zsnr' if z else 'plain'}" for c, p, z in GRID])
def test_host_coefficients_match_restatement(cpu_step, case, pred, zero_snr):
    kind, kw, n = case
    # DPM's sigma table is fp32 (as upstream): the product derives it with fp32 operations, the restatement in fp64,
    # a few fp32 ulps apart; the other schedulers share the alpha-bar table exactly.  Epsilon at a zero-SNR DPM step
    # (alpha_t = 2^-12) stays within that.
    tol = 1e-9 if kind != "dpm" else 4e-6
    worst = [0.0]

    def check(i, got, want):
        for a, b in zip(got, want):
            err = (a.double() - b).abs().max().item()
            scale = b.abs().max().item() + 1.0
            worst[0] = max(worst[0], err / scale)
            assert err <= tol * scale, (i, err, scale)

    for r in (0.0, 0.7):
        s, ref = R.make_pair(kind, n, pred, zero_snr, **kw)
        R.run_teacher_forced(s, ref, kind, (2, 4, 6, 5), 7.5, r, "cpu", check)
    print(f"{kind} {kw} {pred} zsnr={zero_snr}: worst |err| / (max|ref| + 1) {worst[0]:.2e}")


# ------------------------------------------------------------------------------------------------ checkpoint config
SD15_PNDM_JSON = {"_class_name": "PNDMScheduler", "_diffusers_version": "0.6.0", "beta_end": 0.012,
                  "beta_schedule": "scaled_linear", "beta_start": 0.00085, "num_train_timesteps": 1000,
                  "set_alpha_to_one": False, "skip_prk_steps": True, "steps_offset": 1, "trained_betas": None,
                  "clip_sample": False}


def _ckpt(tmp_path, sched_json=None):
    if sched_json is not None:
        os.makedirs(tmp_path / "scheduler", exist_ok=True)
        (tmp_path / "scheduler" / "scheduler_config.json").write_text(json.dumps(sched_json))
    return str(tmp_path)


def test_load_scheduler_config(tmp_path):
    from sonicdiffusionbayeslab_amd.weights import load_scheduler_config
    assert load_scheduler_config(_ckpt(tmp_path / "a")) == SD15_SCHEDULER_CONFIG
    sd15 = load_scheduler_config(_ckpt(tmp_path / "b", SD15_PNDM_JSON))
    assert sd15.pop("_class_name") == "PNDMScheduler" and "_diffusers_version" not in sd15
    accepted = set().union(*(c._accepted for c in (DDIMSchedulerMy, DPMSolverScheduler, LCMScheduler, PNDMScheduler)))
    assert {k: v for k, v in sd15.items() if k in accepted} == \
        {k: v for k, v in SD15_SCHEDULER_CONFIG.items() if k in accepted}
    v = load_scheduler_config(_ckpt(tmp_path / "c", dict(SD15_PNDM_JSON, _class_name="DDIMScheduler",
                                                           prediction_type="v_prediction", rescale_betas_zero_snr=True,
                                                           timestep_spacing="trailing")))
    d = DDIMSchedulerMy.from_config(v)
    assert d.config.prediction_type == "v_prediction" and d.config.rescale_betas_zero_snr and d.alphas_cumprod[-1] == 0


def _method(kind, cfg):
    from sonicdiffusionbayeslab_amd.config import _wrap
    from sonicdiffusionbayeslab_amd.experiments.deep_cache import DeepCacheMethod
    from sonicdiffusionbayeslab_amd.experiments.default_sd import DefaultStableDiffusion
    m = object.__new__(DefaultStableDiffusion if kind == "default" else DeepCacheMethod)
    m.config = _wrap(cfg)
    m.model = type("M", (), {})()
    return m


@pytest.mark.parametrize("kind", ["default", "deep_cache"])
def test_methods_build_the_checkpoint_scheduler_class(tmp_path, kind):
    from sonicdiffusionbayeslab_amd.weights import load_scheduler_config
    for cls_name, want in (("PNDMScheduler", PNDMScheduler), ("DDIMScheduler", DDIMSchedulerMy),
                           ("DPMSolverMultistepScheduler", DPMSolverScheduler), ("LCMScheduler", LCMScheduler)):
        m = _method(kind, {"experiment_params": {}})
        m.model.scheduler = PNDMConfigStub(load_scheduler_config(_ckpt(tmp_path / cls_name,
                                                                        dict(SD15_PNDM_JSON, _class_name=cls_name))))
        m.setup_scheduler()
        assert type(m.model.scheduler) is want
    m = _method(kind, {"experiment_params": {}})              # no file: PNDM, as before
    m.model.scheduler = PNDMConfigStub(load_scheduler_config(_ckpt(tmp_path / "none")))
    m.setup_scheduler()
    assert type(m.model.scheduler) is PNDMScheduler
    m = _method(kind, {"experiment_params": {}})
    m.model.scheduler = PNDMConfigStub(load_scheduler_config(_ckpt(tmp_path / "euler", dict(SD15_PNDM_JSON,
                                                                   _class_name="EulerDiscreteScheduler"))))
    with pytest.raises(NotImplementedError, match="EulerDiscreteScheduler"):
        m.setup_scheduler()
    if kind == "deep_cache":                                  # a YAML scheduler_name still wins
        m = _method(kind, {"experiment_params": {}, "scheduler": {"scheduler_name": "ddim_scheduler"}})
        m.model.scheduler = PNDMConfigStub(load_scheduler_config(_ckpt(tmp_path / "euler")))
        m.setup_scheduler()
        assert type(m.model.scheduler) is DDIMSchedulerMy


def test_from_pretrained_reads_the_checkpoint_scheduler_config(tmp_path, monkeypatch):
    from sonicdiffusionbayeslab_amd import models as M
    monkeypatch.setattr(M, "load_unet_config", lambda p: M.UNetConfig(sample_size=8))
    monkeypatch.setattr(M, "load_unet_state_dict", lambda p: {})
    monkeypatch.delenv("SD_AMD_MODEL_DIR", raising=False)
    m = M.StableDiffusionModel.from_pretrained(_ckpt(tmp_path / "v", dict(SD15_PNDM_JSON, _class_name="DDIMScheduler",
                                                                          prediction_type="v_prediction")))
    assert m.scheduler.config["_class_name"] == "DDIMScheduler" and m.scheduler.config.prediction_type == "v_prediction"
    m = M.StableDiffusionModel.from_pretrained(_ckpt(tmp_path / "plain"))
    assert dict(m.scheduler.config) == SD15_SCHEDULER_CONFIG
    assert dict(M.StableDiffusionModel.from_pretrained("runwayml/stable-diffusion-v1-5").scheduler.config) == \
        SD15_SCHEDULER_CONFIG


def test_yaml_guidance_rescale_reaches_the_call():
    from sonicdiffusionbayeslab_amd.config import _wrap
    from sonicdiffusionbayeslab_amd.experiments.ddim import DDIMMethod
    seen = []
    for ep, want in (({}, None), ({"guidance_rescale": 0.7}, 0.7)):
        m = object.__new__(DDIMMethod)
        m.config = _wrap({"experiment_name": "t", "experiment_params": ep, "inference": {}})
        m.model = type("M", (), {"to": lambda self, d: self})()
        m.device, m.test_dataset, m.last_prompts = "cpu", type("D", (), {"batches": lambda self, b: []})(), []
        m.generate = lambda loader, steps, bs, guidance_scale=7.5, **kw: seen.append(kw) or ([], [])
        m.validate = lambda *a, **k: None
        m.sweep([5], lambda n: {"num_inference_steps": n}, lambda n: "")
        assert seen[-1].get("guidance_rescale") == want and seen[-1]["num_inference_steps"] == 5
