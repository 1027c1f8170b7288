"""UniPC and Karras sigmas without a GPU: the coefficient rows of ``sd_sched_step_pc`` against the fp64 restatement in
tests/unipc_ref.py, against DPM-Solver++ 2M (corrector off), and on an ODE with a closed-form solution; the Karras table;
the harness surface, the refusals and the kernel's argument checks.

The row tests run ``UniPCScheduler.step_fused`` itself (its order logic, history and ``last_sample`` state) with the launch
replaced by a float64 numpy evaluation of the formula documented in include/sd_hip.h::sd_sched_step_pc."""
import ctypes as C
import json
import math
import os

import numpy as np
import pytest
import torch

from sonicdiffusionbayeslab_amd import _lib
from sonicdiffusionbayeslab_amd import schedulers as S
from sonicdiffusionbayeslab_amd.schedulers import (DPMSolverScheduler, PNDMConfigStub, SD15_SCHEDULER_CONFIG, UniPCScheduler,
                                                   unipc_rows)
from tests import sched_ref as R
from tests import unipc_ref as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LINEAR = dict(num_train_timesteps=1000, beta_start=0.0001, beta_end=0.02, beta_schedule="linear")


# ------------------------------------------------------------------------------------------------ the documented formula
def apply_rows(rows, e, x, x_last, hist):
    """include/sd_hip.h::sd_sched_step_pc after the CFG combine, in numpy float64: (prev, xc, y2, m_t)."""
    cm, cy, cc, cp = rows
    for row in (cm, cy, cp) + (() if cc is None else (cc,)):
        assert all(math.isfinite(v) for v in row), rows
    h1, h2, h3 = hist
    m_t = cm[0] * x + cm[1] * e
    y2 = cy[0] * x + cy[1] * e
    if x_last is None:
        xc = x
    else:
        xc = cc[0] * x_last
        for w, h in ((cc[1], h1), (cc[2], h2), (cc[3], h3)):
            if h is not None:
                xc = xc + w * h
            else:
                assert w == 0.0
        xc = xc + cc[4] * m_t
    prev = cp[0] * xc + cp[1] * m_t
    for w, h in ((cp[2], h1), (cp[3], h2)):
        if h is not None:
            prev = prev + w * h
        else:
            assert w == 0.0
    return prev, xc, y2, m_t


def _np(t):
    return None if t is None else t.numpy()


def _cpu_launch_pc(eps, cfg, guidance, x, x_last, hist, rows, k=None, blend=None):
    assert blend is None
    B = x.shape[0]
    e = eps[:B] + guidance * (eps[B:] - eps[:B]) if cfg else eps
    if k is not None:
        e = e * k.view(-1, *([1] * (e.dim() - 1)))
    out = apply_rows(rows, e.numpy(), x.numpy(), _np(x_last), [_np(h) for h in hist])
    return tuple(torch.from_numpy(np.asarray(o, dtype=np.float64)) for o in out)


def _cpu_factors(eps, batch, guidance, rescale):
    u, c = eps.double().chunk(2)
    return R.rescale_factor(R.cfg_combine(u, c, guidance), c, rescale).flatten()


@pytest.fixture
def cpu_pc(monkeypatch):
    monkeypatch.setattr(UniPCScheduler, "_launch_pc", staticmethod(_cpu_launch_pc))
    monkeypatch.setattr(S._FusedStepScheduler, "_prep", staticmethod(lambda t: t.double()))
    monkeypatch.setattr(S, "cfg_rescale_factors", _cpu_factors)


def make_pair(n, base=None, **kw):
    """(UniPCScheduler after set_timesteps(n), the restatement on the product's own sigma table and timesteps)."""
    s = UniPCScheduler.from_config(PNDMConfigStub().config if base is None else base, **kw)
    s.set_timesteps(n)
    c = s.config
    ref = U.UniPC(s.sigmas, s._timesteps_list, c.prediction_type, c.solver_order, c.solver_type, c.predict_x0,
                  c.lower_order_final, c.disable_corrector)
    return s, ref


def rel(a, b):
    return (a.double() - b).abs().max().item() / max(b.abs().max().item(), 1e-300)


def run_schedule(s, ref, start=0, seed=3, shape=(2, 3, 5), free=True):
    """Every step from ``start``: the product's step_fused and the restatement, both free-running from the same start and
    the same model outputs.  Returns the worst relative difference over prev, x0, the corrected sample and the history
    entry."""
    g = torch.Generator().manual_seed(seed)
    xs = xr = torch.randn(shape, generator=g, dtype=torch.float64)
    worst = 0.0
    for t in list(s._timesteps_list)[start:]:
        m = torch.randn(shape, generator=g, dtype=torch.float64)
        got = s.step_fused(m, 0.0, xs, t, cfg=False)
        want = ref.step(m, t, xr)
        for a, b in zip(got + (s.last_sample, s.model_outputs[-1]), want + (ref.last_sample, ref.m_t)):
            assert torch.isfinite(a).all()
            worst = max(worst, rel(a, b))
        xs, xr = got[0], want[0]
    return worst


# ------------------------------------------------------------------------------------------------ 1. rows vs restatement
ROW_GATE = 1e-10      # both sides fp64, differing by association only


@pytest.mark.parametrize("pred", ["epsilon", "v_prediction", "sample"])
@pytest.mark.parametrize("predict_x0", [True, False])
@pytest.mark.parametrize("solver_type", ["bh1", "bh2"])
@pytest.mark.parametrize("order", [1, 2, 3])
def test_rows_match_the_restatement(cpu_pc, order, solver_type, predict_x0, pred):
    worst = 0.0
    for n in (1, 2, 3, 5, 10):
        for final in ("zero", "sigma_min"):
            s, ref = make_pair(n, solver_order=order, solver_type=solver_type, predict_x0=predict_x0, prediction_type=pred,
                               final_sigmas_type=final)
            w = run_schedule(s, ref)
            assert w <= ROW_GATE, (n, final, w)
            worst = max(worst, w)
    print(f"order {order} {solver_type} predict_x0={predict_x0} {pred}: worst relative difference {worst:.2e}")


@pytest.mark.parametrize("kw,start", [
    (dict(rescale_betas_zero_snr=True, prediction_type="v_prediction", timestep_spacing="trailing"), 0),
    (dict(rescale_betas_zero_snr=True, prediction_type="v_prediction"), 0),
    (dict(disable_corrector=[0, 2]), 0),
    (dict(), 3),                                            # image-to-image: the first executed step has no corrector
    (dict(use_karras_sigmas=True), 0),
    (dict(lower_order_final=False, final_sigmas_type="sigma_min"), 0),
], ids=["zsnr-v-trailing", "zsnr-v-linspace", "disable-0-2", "start-3", "karras", "no-lower-order-final"])
@pytest.mark.parametrize("order", [1, 2, 3])
def test_rows_match_the_restatement_special_cases(cpu_pc, order, kw, start):
    for solver_type in ("bh1", "bh2"):
        for n in (5, 10):
            s, ref = make_pair(n, solver_order=order, solver_type=solver_type, **kw)
            w = run_schedule(s, ref, start=start)
            assert w <= ROW_GATE, (solver_type, n, w)
            if start:
                assert ref.i == n and s.step_index == n


def test_step_orders_follow_upstream(cpu_pc):
    """The corrector runs at the previous step's order, never on the first executed step, and not after a disabled step;
    the predictor warms up 1, 2, 3 and comes down 3, 2, 1 under lower_order_final."""
    s, _ = make_pair(8, solver_order=3, disable_corrector=[4])
    seen = []
    x = torch.zeros(1, 4, dtype=torch.float64)
    for i, t in enumerate(s._timesteps_list):
        seen.append(s.step_orders(i))
        s.step_fused(torch.ones_like(x), 0.0, x, t, cfg=False)
    assert seen == [(0, 1), (1, 2), (2, 3), (3, 3), (3, 3), (0, 3), (3, 2), (2, 1)]
    s.set_timesteps(8)                                      # resets history, last_sample, this_order and lower_order_nums
    assert s.last_sample is None and s.model_outputs == [None] * 3 and s.this_order == 0 and s.lower_order_nums == 0
    assert s.step_index is None


def test_step_is_the_drop_in(cpu_pc):
    s, ref = make_pair(4)
    x = torch.randn(1, 4, 2, 2, dtype=torch.float64)
    m = torch.randn(1, 4, 2, 2, dtype=torch.float64)
    got = s.step(m, s._timesteps_list[0], x)
    want = ref.step(m, s._timesteps_list[0], x)
    assert len(got) == 2 and rel(got[0], want[0]) <= ROW_GATE and rel(got[1], want[1]) <= ROW_GATE


def test_a_step_onto_sigma_zero_above_first_order_is_refused():
    s = UniPCScheduler.from_config(PNDMConfigStub().config, lower_order_final=False)
    s.set_timesteps(4)
    with pytest.raises(ValueError, match="sigma 0"):
        unipc_rows(s.sigmas, 3, 2, 2)


# ------------------------------------------------------------------------------------------------ 2. anchor: DPM-Solver++ 2M
ANCHOR_GATE = 1e-12


@pytest.mark.parametrize("final", ["zero", "sigma_min"])
@pytest.mark.parametrize("n", [2, 5, 10, 20])
@pytest.mark.parametrize("order", [1, 2])
def test_corrector_off_is_dpm_solver_pp_midpoint(order, n, final):
    base = PNDMConfigStub().config
    u = UniPCScheduler.from_config(base, solver_order=order, solver_type="bh2", predict_x0=True, final_sigmas_type=final,
                                   disable_corrector=list(range(n)))
    d = DPMSolverScheduler.from_config(base, solver_order=order, algorithm_type="dpmsolver++", solver_type="midpoint",
                                       final_sigmas_type=final)
    u.set_timesteps(n)
    d.set_timesteps(n)
    assert u.sigmas.tobytes() == d.sigmas.tobytes() and u._timesteps_list == d._timesteps_list
    g = torch.Generator().manual_seed(11)
    xu = xd = torch.randn((2, 7), generator=g, dtype=torch.float64).numpy()
    hu, hd = [], []                                         # histories, newest first
    lower = 0
    for i in range(n):
        e = torch.randn((2, 7), generator=g, dtype=torch.float64).numpy()
        o = min(min(order, n - i), lower + 1)               # UniPC's order of this step; DPM's update is asked for the same
        rows = unipc_rows(u.sigmas, i, 0, o, "bh2", True, "epsilon")
        prev_u, xc, x0_u, m_u = apply_rows(rows, e, xu, None, (hu + [None] * 3)[:3] if o > 1 else [None] * 3)
        assert xc is xu
        yx, ye, mx, me = d._convert_coefs(i)
        px, pe, p1, p2, pn = d._update_coefs(i, o, mx, me)
        assert pn == 0.0 and p2 == 0.0
        prev_d = px * xd + pe * e + (p1 * hd[0] if o > 1 else 0.0)
        m_d = mx * xd + me * e
        for a, b in ((prev_u, prev_d), (m_u, m_d), (x0_u, yx * xd + ye * e)):
            assert np.abs(a - b).max() <= ANCHOR_GATE * np.abs(b).max(), (i, np.abs(a - b).max() / np.abs(b).max())
        hu, hd = [m_u] + hu, [m_d] + hd
        xu, xd = prev_u, prev_d
        lower = min(lower + 1, order)


# ------------------------------------------------------------------------------------------------ 3. order of accuracy
# Gaussian data of variance 0.25: eps(x, sigma) = s x / (0.25 a^2 + s^2), a = 1 / sqrt(1 + sigma^2), s = sigma a, and the
# probability-flow ODE has the solution x(sigma) = x_T sqrt((0.25 a^2 + s^2) / (0.25 a_T^2 + s_T^2)).
def _gauss(sigma):
    a = 1.0 / math.sqrt(1.0 + sigma * sigma)
    return a, sigma * a, 0.25 * a * a + (sigma * a) ** 2


def _ode_error(N, order, solver_type, corrector, monkeypatch):
    sig = np.exp(np.linspace(math.log(10.0), math.log(0.1), N + 1))
    s = UniPCScheduler.from_config(LINEAR, solver_order=order, solver_type=solver_type, lower_order_final=False,
                                   final_sigmas_type="sigma_min", disable_corrector=[] if corrector else list(range(N)))
    s.set_timesteps(N)
    s.sigmas = sig                                          # the custom table, fp64 (the row function takes any table)
    x = torch.ones(1, 4, dtype=torch.float64)
    for i, t in enumerate(s._timesteps_list):
        _, sg, v = _gauss(sig[i])
        x, _ = s.step_fused(sg * x / v, 0.0, x, t, cfg=False)
    exact = math.sqrt(_gauss(sig[-1])[2] / _gauss(sig[0])[2])
    return abs(x[0, 0].item() - exact) / exact


@pytest.mark.parametrize("solver_type,order,corrector", [("bh2", 1, False), ("bh2", 2, False), ("bh2", 3, False),
                                                         ("bh2", 1, True), ("bh2", 2, True), ("bh2", 3, True),
                                                         ("bh1", 2, False), ("bh1", 3, False),
                                                         ("bh1", 2, True), ("bh1", 3, True)])
def test_order_of_accuracy_on_a_gaussian(cpu_pc, monkeypatch, solver_type, order, corrector):
    """The predictor alone at order p converges at >= p - 0.5, predictor plus corrector at >= p + 1 - 0.5, on a grid uniform
    in log sigma from 10 to 0.1 (conditions, not measurements; the restatement's own observed orders, for reference:
    P 0.99 / 1.94-1.97 / 4.1-4.2, PC 2.00 / 3.00 / 3.8-3.9 for bh2 orders 1 / 2 / 3)."""
    err = {N: _ode_error(N, order, solver_type, corrector, monkeypatch) for N in (32, 64, 128)}
    need = order + (1 if corrector else 0) - 0.5
    for N in (32, 64):
        observed = math.log2(err[N] / err[2 * N])
        print(f"{solver_type} order {order} {'PC' if corrector else 'P'}: N {N} -> {2 * N}: observed order {observed:.2f}")
        assert observed >= need, (N, observed, need, err)


# ------------------------------------------------------------------------------------------------ 4. Karras sigmas
@pytest.mark.parametrize("base", [SD15_SCHEDULER_CONFIG, LINEAR], ids=["sd15", "linear"])
@pytest.mark.parametrize("n", [5, 10, 20, 50])
@pytest.mark.parametrize("cls", [UniPCScheduler, DPMSolverScheduler])
def test_karras_table(cls, n, base):
    for final in ("zero", "sigma_min"):
        s = cls.from_config(base, use_karras_sigmas=True, final_sigmas_type=final, timestep_spacing="trailing")
        s.set_timesteps(n)
        assert s.sigmas.dtype == np.float32 and len(s.sigmas) == n + 1
        ts, sig = U.karras_table(torch.from_numpy(s.alphas_cumprod), n, final)
        assert s._timesteps_list == ts
        got, want = s.sigmas.astype(np.float64), np.array(sig)
        assert (np.abs(got - want) <= 1e-6 * np.abs(want)).all(), np.abs(got / np.where(want == 0, 1, want) - 1).max()
        t = s._timesteps_list
        assert all(a >= b for a, b in zip(t, t[1:])) and t[0] == 999 and t[-1] == 0
        assert s.timesteps.tolist() == t
        # timestep_spacing is not read in this mode
        o = cls.from_config(base, use_karras_sigmas=True, final_sigmas_type=final, timestep_spacing="leading")
        o.set_timesteps(n)
        assert o.sigmas.tobytes() == s.sigmas.tobytes() and o._timesteps_list == t
    with pytest.raises(ValueError, match="use_karras_sigmas"):
        s.set_timesteps(timesteps=[999, 500, 0])


def test_dpm_tables_without_the_key_are_unchanged():
    """With ``use_karras_sigmas`` False or absent DPMSolverScheduler builds the tables it built before the key existed: the
    expression of its ``set_timesteps`` restated here, byte for byte."""
    assert DPMSolverScheduler.from_config(SD15_SCHEDULER_CONFIG).config.use_karras_sigmas is False
    for base in (SD15_SCHEDULER_CONFIG, LINEAR):
        for spacing in ("linspace", "leading", "trailing"):
            for final in ("zero", "sigma_min"):
                for n in (1, 7, 20, 50):
                    a = DPMSolverScheduler.from_config(base, timestep_spacing=spacing, final_sigmas_type=final)
                    b = DPMSolverScheduler.from_config(base, timestep_spacing=spacing, final_sigmas_type=final,
                                                       use_karras_sigmas=False)
                    a.set_timesteps(n)
                    b.set_timesteps(n)
                    assert a.sigmas.tobytes() == b.sigmas.tobytes() and a._timesteps_list == b._timesteps_list
                    ac = a.alphas_cumprod
                    if spacing == "linspace":
                        ts = np.linspace(0, 999, n + 1).round()[::-1][:-1].copy().astype(np.int64)
                    elif spacing == "leading":
                        ts = (np.arange(0, n + 1) * (1000 // (n + 1))).round()[::-1][:-1].copy().astype(np.int64) \
                            + a.config.steps_offset
                    else:
                        ts = np.arange(1000, 0, -1000 / n).round().copy().astype(np.int64) - 1
                    sig = np.interp(ts, np.arange(0, 1000), np.array(((1 - ac) / ac) ** 0.5))
                    last = ((1 - ac[0]) / ac[0]) ** 0.5 if final == "sigma_min" else 0
                    want = np.concatenate([sig, [last]]).astype(np.float32)
                    assert a.sigmas.tobytes() == want.tobytes() and a._timesteps_list == [int(t) for t in ts]


def test_add_noise_coefs_come_from_the_sigma_table():
    s = UniPCScheduler.from_config(PNDMConfigStub().config, use_karras_sigmas=True)
    s.set_timesteps(10)
    i = 4
    a, sg = s._add_noise_coefs(s._timesteps_list[i])
    sigma = float(s.sigmas[i])
    assert a == 1.0 / math.sqrt(sigma * sigma + 1.0) and sg == sigma * a


# ------------------------------------------------------------------------------------------------ 5. surface
def test_registry_loader_yaml_and_method(tmp_path):
    import sonicdiffusionbayeslab_amd as pkg
    from sonicdiffusionbayeslab_amd.config import load_named_config
    from sonicdiffusionbayeslab_amd.experiments.unipc import UniPCMethod
    from sonicdiffusionbayeslab_amd.weights import load_scheduler_config
    assert pkg.schedulers_registry["unipc_scheduler"] is UniPCScheduler
    assert pkg.methods_registry["unipc"] is UniPCMethod
    assert S.CHECKPOINT_SCHEDULERS["UniPCMultistepScheduler"] == "unipc_scheduler"
    os.makedirs(tmp_path / "scheduler")
    (tmp_path / "scheduler" / "scheduler_config.json").write_text(json.dumps({
        "_class_name": "UniPCMultistepScheduler", "_diffusers_version": "0.32.1", "beta_end": 0.012,
        "beta_schedule": "scaled_linear", "beta_start": 0.00085, "num_train_timesteps": 1000, "solver_order": 3,
        "solver_type": "bh1", "predict_x0": True, "disable_corrector": [1], "prediction_type": "v_prediction",
        "use_karras_sigmas": True, "lower_order_final": True, "thresholding": False, "sample_max_value": 1.0,
        "timestep_spacing": "trailing", "steps_offset": 1, "solver_p": None, "final_sigmas_type": "sigma_min"}))
    conf = load_scheduler_config(str(tmp_path))
    assert S.checkpoint_scheduler_name(conf) == "unipc_scheduler"
    s = pkg.schedulers_registry[S.checkpoint_scheduler_name(conf)].from_config(conf)
    c = s.config
    assert type(s) is UniPCScheduler and (c.solver_order, c.solver_type, c.disable_corrector) == (3, "bh1", [1])
    assert c.prediction_type == "v_prediction" and c.use_karras_sigmas is True and c.final_sigmas_type == "sigma_min"
    assert "sample_max_value" not in c and "_class_name" not in c
    d = UniPCScheduler.from_config(SD15_SCHEDULER_CONFIG).config             # defaults over a PNDM checkpoint config
    assert (d.solver_order, d.solver_type, d.predict_x0, d.lower_order_final, d.disable_corrector, d.final_sigmas_type,
            d.use_karras_sigmas, d.thresholding) == (2, "bh2", True, True, [], "zero", False, False)

    cfg = load_named_config("unipc_config.yaml", os.path.join(ROOT, "configs"))
    assert cfg.experiment.method == "unipc" and cfg.scheduler.scheduler_name == "unipc_scheduler"
    assert list(cfg.experiment_params.num_inference_steps) == [5, 8, 10, 15, 20]
    assert cfg.experiment_params.solver_order == 2 and cfg.experiment_params.solver_type == "bh2"


def _method(cls, ep):
    from sonicdiffusionbayeslab_amd.config import _wrap
    m = object.__new__(cls)
    m.config = _wrap({"experiment_params": ep, "scheduler": {"scheduler_name": {"UniPCMethod": "unipc_scheduler"}.get(
        cls.__name__, "dpm_solver_scheduler")}})
    m.model = type("M", (), {})()
    m.model.scheduler = PNDMConfigStub()
    m.setup_exp_params()
    m.setup_scheduler()
    return m.model.scheduler


def test_methods_pass_their_keys_to_the_scheduler():
    from sonicdiffusionbayeslab_amd.experiments.dpm_solver import DPMSolverMethod
    from sonicdiffusionbayeslab_amd.experiments.unipc import UniPCMethod
    s = _method(UniPCMethod, {"solver_order": 3, "num_inference_steps": [5]})
    assert type(s) is UniPCScheduler and s.config.solver_order == 3 and s.config.solver_type == "bh2"
    s = _method(UniPCMethod, {"solver_order": 2, "num_inference_steps": [5], "solver_type": "bh1", "predict_x0": False,
                              "disable_corrector": [0], "use_karras_sigmas": True, "final_sigmas_type": "sigma_min"})
    c = s.config
    assert (c.solver_type, c.predict_x0, c.disable_corrector, c.use_karras_sigmas, c.final_sigmas_type) == \
        ("bh1", False, [0], True, "sigma_min")
    d = _method(DPMSolverMethod, {"solver_order": 2, "num_inference_steps": [5]})
    assert type(d) is DPMSolverScheduler and d.config.use_karras_sigmas is False
    d = _method(DPMSolverMethod, {"solver_order": 2, "num_inference_steps": [5], "use_karras_sigmas": True})
    assert d.config.use_karras_sigmas is True


def test_export_is_declared_with_the_headers_arity():
    lib = _lib.load()
    n = "sd_sched_step_pc"
    assert hasattr(lib, n) and n in _lib._SIGS and n in _lib.declared_symbols()
    src = open(_lib.HEADER_PATH).read()
    decl = src[src.index("int sd_sched_step_pc("):]
    decl = decl[:decl.index(";")]
    assert len(_lib._SIGS[n][1]) == decl.count(",") + 1 == 23
    assert lib.sd_abi_version() == 3


def test_refusals_name_their_reason_before_any_gpu_work(monkeypatch):
    from sonicdiffusionbayeslab_amd import models as M
    base = PNDMConfigStub().config
    with pytest.raises(NotImplementedError, match="thresholding"):
        UniPCScheduler.from_config(base, thresholding=True)
    with pytest.raises(NotImplementedError, match="solver_type 'logrho'"):
        UniPCScheduler.from_config(base, solver_type="logrho")
    with pytest.raises(ValueError, match="solver_order=4"):
        UniPCScheduler.from_config(base, solver_order=4)
    with pytest.raises(NotImplementedError, match="flow_prediction"):
        UniPCScheduler.from_config(base, prediction_type="flow_prediction")
    with pytest.raises(ValueError, match="epsilon.*rescale_betas_zero_snr.*trailing"):
        UniPCScheduler.from_config(base, rescale_betas_zero_snr=True, timestep_spacing="trailing").set_timesteps(10)
    with pytest.raises(ValueError, match="epsilon"):
        UniPCScheduler.from_config(base, rescale_betas_zero_snr=True, use_karras_sigmas=True).set_timesteps(10)
    UniPCScheduler.from_config(base, rescale_betas_zero_snr=True, timestep_spacing="leading").set_timesteps(10)
    UniPCScheduler.from_config(base, rescale_betas_zero_snr=True, timestep_spacing="trailing",
                               prediction_type="v_prediction").set_timesteps(10)
    with pytest.raises(_lib.SdHipError, match="GPU"):       # a CPU tensor never reaches the launch
        s = UniPCScheduler.from_config(base)
        s.set_timesteps(4)
        s.step_fused(torch.zeros(2, 4, 8, 8), 7.5, torch.zeros(1, 4, 8, 8), s._timesteps_list[0])

    # the three variant pipelines, before any GPU work: every GPU-facing piece raises if it is reached
    def boom(*a, **k):
        raise AssertionError("reached GPU work")
    monkeypatch.setattr(M.StableDiffusionModel, "_begin", boom)
    cfg = M.UNetConfig(sample_size=8)
    uni, ddim = UniPCScheduler.from_config(base), S.DDIMSchedulerMy.from_config(base)
    two = M.StableDiffusionModelTwoSchedulers(unet_config=cfg, state_dict={})
    for first, second in ((uni, ddim), (ddim, uni)):
        two.scheduler_first, two.scheduler_second = first, second
        with pytest.raises(NotImplementedError, match="UniPCScheduler.*StableDiffusionModelTwoSchedulers"):
            two.call(prompt=["a"])
    inter = M.StableDiffusionModelInterlivingSchedulers(unet_config=cfg, state_dict={})
    inter.scheduler_main, inter.scheduler_inter = uni, ddim
    with pytest.raises(NotImplementedError, match="UniPCScheduler.*StableDiffusionModelInterlivingSchedulers"):
        inter.call(prompt=["a"])
    skip = M.StableDiffusionModelSkipTimesteps(unet_config=cfg, state_dict={})
    skip.scheduler = uni
    with pytest.raises(NotImplementedError, match="UniPCScheduler.*StableDiffusionModelSkipTimesteps"):
        skip.call(prompt=["a"], skip_timesteps=[1])


# ------------------------------------------------------------------------------------------------ 6. kernel argument checks
def _pc(lib, **kw):
    """sd_sched_step_pc with a NULL stream and never-dereferenced addresses: every call here fails in a host-side check."""
    n = kw.pop("n", 256)
    a = dict(eps=0x10000, cfg=0, guidance=1.0, x=0x20000, x_last=None, h1=None, h2=None, h3=None, prev=0x30000, x_corr=None,
             y2=None, m_out=None, coef=(C.c_float * 13)(), n=n, k=None, nps=n, init=None, blend_noise=None, mask=None, a=1.0,
             s=0.0, hw=0)
    a.update(kw)
    rc = lib.sd_sched_step_pc(None, a["eps"], a["cfg"], a["guidance"], a["x"], a["x_last"], a["h1"], a["h2"], a["h3"],
                              a["prev"], a["x_corr"], a["y2"], a["m_out"], a["coef"], a["n"], a["k"], a["nps"], a["init"],
                              a["blend_noise"], a["mask"], a["a"], a["s"], a["hw"])
    return rc, lib.sd_last_error().decode()


def _coef(**at):
    c = (C.c_float * 13)()
    for i, v in at.items():
        c[int(i[1:])] = v
    return c


def test_kernel_argument_checks_refuse_without_a_launch():
    lib = _lib.load()
    for null in ("eps", "x", "prev", "coef"):
        rc, msg = _pc(lib, **{null: None})
        assert rc != 0 and "null" in msg, (null, msg)
    for n in (0, -4, 6, 255):
        rc, msg = _pc(lib, n=n)
        assert rc != 0 and "positive multiple of 4" in msg, (n, msg)
    for nps in (0, 6, 100, 96):                             # % 4, and dividing n = 256
        rc, msg = _pc(lib, nps=nps)
        assert rc != 0 and "n_per_sample" in msg, (nps, msg)
    # the blend: the argument checks of sd_sched_step_inpaint
    blend = dict(init=0x40000, blend_noise=0x50000, mask=0x60000, a=0.5, s=0.5, hw=64)
    for bad, word in ((dict(hw=6), "hw"), (dict(hw=0), "hw"), (dict(hw=48), "hw"), (dict(mask=None), "mask"),
                      (dict(blend_noise=None), "blend_noise"), (dict(a=float("inf")), "finite"), (dict(s=float("nan")), "finite")):
        rc, msg = _pc(lib, **dict(blend, **bad))
        assert rc != 0 and word in msg, (bad, msg)
    # every coefficient is finite
    for j in range(13):
        for v in (float("inf"), float("nan")):
            rc, msg = _pc(lib, coef=_coef(**{f"c{j}": v}))
            assert rc != 0 and "finite" in msg, (j, msg)
    rc, msg = _pc(lib, guidance=float("nan"))
    assert rc != 0 and "guidance" in msg
    # a null history entry has no weight: cp2 / cp3 always, cc1..cc3 when the corrector runs
    for j, name in ((11, "h1"), (12, "h2")):
        rc, msg = _pc(lib, coef=_coef(**{f"c{j}": 1.0}))
        assert rc != 0 and f"{name} is null" in msg, msg
    for j, name in ((5, "h1"), (6, "h2"), (7, "h3")):
        rc, msg = _pc(lib, coef=_coef(**{f"c{j}": 1.0}), x_last=0x70000)
        assert rc != 0 and f"{name} is null" in msg, msg
    # an output that aliases an input, or another output, by name (overlap counts: 0x20000 + 512 lies inside x)
    for out in ("prev", "x_corr", "y2", "m_out"):
        for inp, extra in (("eps", {}), ("x", {}), ("x_last", {}), ("h1", {}), ("h2", {}), ("h3", {}), ("k", {}),
                           ("init", dict(blend)), ("blend_noise", dict(blend)), ("mask", dict(blend))):
            kw = dict(extra)
            kw.setdefault(inp, 0x80000)
            addr = kw[inp]
            kw[out] = addr
            rc, msg = _pc(lib, **kw)
            assert rc != 0 and f"output {out} aliases input {inp}" in msg, (out, inp, msg)
    rc, msg = _pc(lib, prev=0x20000 + 512)
    assert rc != 0 and "output prev aliases input x" in msg
    rc, msg = _pc(lib, cfg=1, prev=0x10000 + 1024)          # with CFG eps is 2n floats long
    assert rc != 0 and "output prev aliases input eps" in msg
    rc, msg = _pc(lib, y2=0x30000)
    assert rc != 0 and "output y2 aliases output prev" in msg
