"""CPU: what a plain ``bench.py`` run does next to a ``--full`` one.  The model, the timed runs and every extra report are
stand-ins (no GPU here): a plain run must print the headline line and call none of the extras; ``--full`` calls each of
them, and each ``--no-*`` option still leaves its own out."""
import json
import sys
import types

import pytest
import torch

import bench
from sonicdiffusionbayeslab_amd import dist as sdist
from sonicdiffusionbayeslab_amd import models, weights

EXTRAS = ("other_configs", "end_to_end", "gpu_free_running", "cpu_baseline", "full_length_parity", "conv_stream_ceiling")
HEADLINE_KEYS = {"metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"}
FULL_KEYS = {"roofline", "kernel_breakdown", "other_configs", "cpu_baseline"}
FULL_CONFIG_KEYS = {"end_to_end", "parity", "parity_full_length"}


class _FakeUNet:
    def __init__(self, calls):
        self.calls = calls

    def forward_profiled(self, lat, ub, t):
        self.calls.append("forward_profiled")
        return {"conv3x3": {"ms": 1.0, "launches": 44, "flops": 1e12, "bytes": 1e9}}


class _FakeModel:
    calls = None

    def __init__(self, **kw):
        self.unet = _FakeUNet(_FakeModel.calls)
        self.unet_config = kw["unet_config"]

    def to(self, dev):
        return self


def _run(monkeypatch, capsys, *argv):
    calls = []
    _FakeModel.calls = calls
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "2", "--warmup", "1", *argv])
    monkeypatch.setattr(sdist, "init_process_group", lambda backend: (0, 0, 1))
    monkeypatch.setattr(torch.cuda, "set_device", lambda i: None)
    monkeypatch.setattr(weights, "make_synthetic_state_dict", lambda cfg, seed: {})
    monkeypatch.setattr(models, "StableDiffusionModel", _FakeModel)
    lat = torch.zeros((8, 4, 64, 64))
    monkeypatch.setattr(bench, "timed_runs", lambda *a: (calls.append("timed_runs") or (11.0, 700.0, 1.3, lat, 7.5, lat)))
    fakes = {"other_configs": [], "end_to_end": {}, "gpu_free_running": [], "cpu_baseline": ({}, {}),
             "full_length_parity": {}, "conv_stream_ceiling": {}}
    for name in EXTRAS:
        monkeypatch.setattr(bench, name, lambda *a, _n=name, **k: (calls.append(_n) or fakes[_n]))
    bench.main()
    line = capsys.readouterr().out.strip().splitlines()[-1]
    return json.loads(line), calls


def test_plain_run_reports_the_headline_only(monkeypatch, capsys):
    res, calls = _run(monkeypatch, capsys)
    assert calls == ["timed_runs"]
    assert HEADLINE_KEYS <= set(res) and not FULL_KEYS & set(res) and not FULL_CONFIG_KEYS & set(res["config"])
    assert res["value"] == 11.0 and res["ms_per_step"] == 700.0 and res["unit"] == "images/s" and res["dtype"] == "bf16"


def test_full_run_adds_every_extra(monkeypatch, capsys):
    res, calls = _run(monkeypatch, capsys, "--full")
    assert calls[0] == "timed_runs" and set(calls[1:]) == set(EXTRAS) | {"forward_profiled"}
    assert HEADLINE_KEYS | FULL_KEYS <= set(res) and FULL_CONFIG_KEYS <= set(res["config"])


@pytest.mark.parametrize("opt,gone", [("--no-roofline", {"forward_profiled", "conv_stream_ceiling"}),
                                      ("--no-other-configs", {"other_configs"}), ("--no-e2e", {"end_to_end"}),
                                      ("--no-cpu-baseline", {"gpu_free_running", "cpu_baseline"}),
                                      ("--no-parity-full-length", {"full_length_parity"})])
def test_full_run_still_honours_each_no_option(monkeypatch, capsys, opt, gone):
    _, calls = _run(monkeypatch, capsys, "--full", opt)
    assert set(calls[1:]) == (set(EXTRAS) | {"forward_profiled"}) - gone
