"""Perturbed-attention guidance without a GPU: layer names -> masks on three UNet shapes, the adaptive-scale rule, every refusal by
name, the registry key and YAML keys, the exported symbols and the identity op's shape rule, ``pag_scale = 0`` as the plain call,
and the oracle (tests/pag_oracle.py): off it is the plain oracle, and its own perturbed-against-cond distance clears the floor at
every UNet case of the GPU tests."""
import os

import pytest
import torch

from sonicdiffusionbayeslab_amd import _lib
from tests import pag_oracle as po

NEW_SYMBOLS = ["sd_unet_set_pag", "sd_unet_pag_block_count", "sd_pag_identity_check", "sd_op_pag_identity", "sd_sched_step_pag",
               "sd_sched_step_pc_pag", "sd_cfg_rescale_factors_pag"]


# ---------------------------------------------------------------------------------------------------------- layer names
def _cfgs():
    from sonicdiffusionbayeslab_amd.weights import UNetConfig, sd2_unet_config
    return (UNetConfig(sample_size=16), sd2_unet_config(16),
            UNetConfig(sample_size=32, block_out_channels=(320, 640), attn_levels=(True, True)))


def test_layer_names_give_the_mask_by_hand():
    from sonicdiffusionbayeslab_amd.unet import HipUNet2DConditionModel as U
    sd15, sd2, two = _cfgs()
    # sd15 / sd2: 2 + 2 + 2 down blocks (bits 0..5), mid (bit 6), 3 + 3 + 3 up blocks of up_blocks 1..3 (bits 7..15)
    for cfg in (sd15, sd2):
        names = U.pag_block_names(cfg)
        assert len(names) == 16 and names[0] == "down.block_0.attentions_0" and names[6] == "mid" and names[7] == "up.block_1.attentions_0"
        assert names[15] == "up.block_3.attentions_2"
        assert U.pag_layer_mask(cfg, "mid") == 1 << 6
        assert U.pag_layer_mask(cfg, ["mid"]) == 1 << 6
        assert U.pag_layer_mask(cfg, "down.block_0") == 0b11
        assert U.pag_layer_mask(cfg, "down.block_0.attentions_0") == 0b1
        assert U.pag_layer_mask(cfg, "down.block_2.attentions_1") == 1 << 5
        assert U.pag_layer_mask(cfg, "up.block_1") == 0b111 << 7
        assert U.pag_layer_mask(cfg, "up.block_3.attentions_2") == 1 << 15
        assert U.pag_layer_mask(cfg, ["mid", "up.block_1"]) == (1 << 6) | (0b111 << 7)
        assert U.pag_layer_mask(cfg, ("down.block_2", "mid", "up.block_1", "mid")) == (0b11 << 4) | (1 << 6) | (0b111 << 7)
        for bad in ("down.block_3", "up.block_0", "up.block_0.attentions_0", "down.block_0.attentions_2", "up.block_1.attentions_3",
                    "middle", "mid.attentions_0", "down", "down.block_1.", "", None, 3):
            with pytest.raises(ValueError, match="valid names") as e:
                U.pag_layer_mask(cfg, [bad])
            assert "'mid'" in str(e.value) and "down.block_2" in str(e.value)
        with pytest.raises(ValueError, match="empty"):
            U.pag_layer_mask(cfg, [])
    # two levels, attention on both: 2 + 2 down, mid, 3 + 3 up = 11 blocks
    names = U.pag_block_names(two)
    assert len(names) == 11 and names[4] == "mid" and names[5] == "up.block_0.attentions_0"
    assert U.pag_layer_mask(two, ["down.block_0", "up.block_1"]) == 0b11 | (0b111 << 8)
    assert U.pag_layer_mask(two, "up.block_0") == 0b111 << 5
    with pytest.raises(ValueError, match="valid names"):
        U.pag_layer_mask(two, "down.block_2")
    # the oracle's own restatement agrees on every single name and on the GPU file's cases
    for cfg in (sd15, sd2, two):
        for k, name in enumerate(U.pag_block_names(cfg)):
            assert po.layer_mask(cfg, name) == 1 << k == U.pag_layer_mask(cfg, name)
    for case in po.UNET_CASES + [po.SD2_CASE, po.HT_CASE, po.MID_CASE, po.HM_CASE]:
        cfg = po.env(case[0])[0]
        assert bin(U.pag_layer_mask(cfg, list(case[6]))).count("1") == case[7] and U.pag_layer_mask(cfg, list(case[6])) == po.layer_mask(cfg, case[6])


def test_adaptive_scale_rule():
    from sonicdiffusionbayeslab_amd.schedulers import pag_step_scale
    assert pag_step_scale(3.0, 0.0, 981) == 3.0 and pag_step_scale(3.0, 0, 1) == 3.0
    assert pag_step_scale(3.0, 0.005, 1000) == 3.0
    assert pag_step_scale(3.0, 0.005, 800) == pytest.approx(2.0) and pag_step_scale(3.0, 0.005, 400) == pytest.approx(0.0)
    assert pag_step_scale(3.0, 0.005, 399) == 0.0 and pag_step_scale(3.0, 0.005, 1) == 0.0       # clamped, never negative
    assert pag_step_scale(3.0, 0.01, 981) == pytest.approx(2.81)
    for t in (999, 981, 501, 21, 1):
        assert pag_step_scale(3.0, 0.004, t) == po.step_scale(3.0, 0.004, t) == max(3.0 - 0.004 * (1000 - t), 0.0)


# ------------------------------------------------------------------------------------------------- registry, YAML, refusals
def test_registry_key_and_yaml_keys():
    from sonicdiffusionbayeslab_amd.config import _wrap, load_config
    from sonicdiffusionbayeslab_amd.experiments.base_experiment import BaseMethod
    from sonicdiffusionbayeslab_amd.registry import methods_registry
    assert "pag" in methods_registry
    cfg = load_config(os.path.join(os.path.dirname(__file__), "..", "configs", "pag_config.yaml"))
    assert cfg.experiment.method == "pag" and list(cfg.experiment_params.pag_scale) == [None, 3.0]
    assert list(cfg.experiment_params.pag_applied_layers) == ["mid"] and cfg.scheduler.scheduler_name == "ddim_scheduler"
    assert BaseMethod.parse_pag(_wrap({"model_name": "x"})) is None
    assert BaseMethod.parse_pag(_wrap({"pag": {}})) == dict(pag_scale=3.0, pag_adaptive_scale=0.0, pag_applied_layers="mid")
    assert BaseMethod.parse_pag(_wrap({"pag": {"scale": 2, "adaptive_scale": 0.01, "applied_layers": ["mid", "up.block_1"]}})) == \
        dict(pag_scale=2, pag_adaptive_scale=0.01, pag_applied_layers=["mid", "up.block_1"])
    with pytest.raises(ValueError, match="mapping"):
        BaseMethod.parse_pag(_wrap({"pag": 3.0}))
    with pytest.raises(ValueError, match="keys"):
        BaseMethod.parse_pag(_wrap({"pag": {"pag_scale": 3.0}}))
    with pytest.raises(ValueError, match="pag_scale"):
        BaseMethod.parse_pag(_wrap({"pag": {"scale": "3"}}))
    with pytest.raises(ValueError, match="pag_adaptive_scale"):
        BaseMethod.parse_pag(_wrap({"pag": {"adaptive_scale": -0.1}}))
    with pytest.raises(NotImplementedError, match="fp8"):
        BaseMethod.parse_pag(_wrap({"pag": {"scale": 3.0}}), "fp8")


def test_every_refusal_by_name_before_any_gpu_work():
    import dataclasses
    from sonicdiffusionbayeslab_amd.models import (StableDiffusionModel as M, StableDiffusionModelInterlivingSchedulers,
                                                   StableDiffusionModelSkipTimesteps, StableDiffusionModelTwoSchedulers)
    from sonicdiffusionbayeslab_amd.weights import UNetConfig
    m = M()
    for bad in ("3", None, True, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="pag_scale"):
            m.enable_pag(pag_scale=bad)
    for bad in ("0", None, True, float("nan"), -0.001):
        with pytest.raises(ValueError, match="pag_adaptive_scale"):
            m.enable_pag(pag_adaptive_scale=bad)
    with pytest.raises(ValueError, match="valid names"):
        m.enable_pag(pag_applied_layers="down.block_3")
    with pytest.raises(NotImplementedError, match="fp8"):
        M(weight_dtype="fp8").enable_pag()
    with pytest.raises(NotImplementedError, match="9-channel"):
        M(unet_config=dataclasses.replace(UNetConfig(sample_size=16), in_channels=9)).enable_pag()
    assert m._pag is None                                            # nothing above took effect
    for V in (StableDiffusionModelTwoSchedulers, StableDiffusionModelInterlivingSchedulers, StableDiffusionModelSkipTimesteps):
        with pytest.raises(NotImplementedError, match="variant pipelines"):
            V().enable_pag()
        with pytest.raises(NotImplementedError, match="variant pipelines"):
            V().call(prompt="a", pag_scale=3.0)
    # the call's own kwargs without enable_pag
    with pytest.raises(ValueError, match="enable_pag"):
        m._pag_check_call(3.0, None)
    assert m._pag_check_call(None, None) is None
    assert m.enable_pag() is m and m._pag == dict(scale=3.0, adaptive_scale=0.0, layers=["mid"], mask=1 << 6)
    assert m._pag_check_call(None, None) == (3.0, 0.0) and m._pag_check_call(1.5, 0.01) == (1.5, 0.01)
    assert m._pag_check_call(None, 0.02) == (3.0, 0.02)
    with pytest.raises(ValueError, match="pag_scale"):
        m._pag_check_call("1", None)
    # what a PAG call refuses: Token Merging, T-GATE, DeepCache, IP-Adapter, ControlNet
    m.apply_tome(ratio=0.5)
    with pytest.raises(NotImplementedError, match="Token Merging"):
        m._pag_check_call(None, None)
    m.remove_tome()
    m.enable_tgate(2)
    with pytest.raises(NotImplementedError, match="T-GATE"):
        m._pag_check_call(None, None)
    m.disable_tgate()
    m._deepcache = object()
    with pytest.raises(NotImplementedError, match="DeepCache"):
        m._pag_check_call(None, None)
    m._deepcache = None
    with pytest.raises(NotImplementedError, match="ControlNet"):
        m._pag_check_call(None, None, control=torch.zeros(1, 3, 8, 8))
    with pytest.raises(NotImplementedError, match="IP-Adapter"):
        m._pag_check_call(None, None, ip_adapter_image_embeds=torch.zeros(1, 8))
    with pytest.raises(NotImplementedError, match="IP-Adapter"):
        m._pag_check_call(None, None, ip_adapter_image=torch.zeros(1, 3, 8, 8))
    # ... and none of them refuses a call whose scale is 0: that is the plain pipeline
    m.apply_tome(ratio=0.5)
    assert m._pag_check_call(0.0, None) is None
    m.remove_tome()
    assert m.disable_pag() is m and m._pag is None


def test_pag_scale_zero_keys_the_plain_plan():
    """``pag_scale <= 0`` (the default's or the call's) is a plain call: no third prompt row, no layer mask on the UNet handle
    -- so the plan key is the plain one -- and no ``pag_scale`` in the step."""
    from sonicdiffusionbayeslab_amd.models import StableDiffusionModel as M

    class Unet:
        _pag = 0

        def __init__(self):
            self.calls = []

        def set_pag(self, mask):
            self.calls.append(mask)
            self._pag = mask
    m = M().enable_pag(pag_scale=3.0, pag_applied_layers=["mid", "up.block_1"])
    m.unet = Unet()
    for scale in (0.0, -1.0):
        m._pag_call = m._pag_check_call(scale, None)
        assert m._pag_call is None
        m._pag_begin()
        assert m.unet.calls == []                                    # a handle that never had a mask is not touched
    m._pag_call = m._pag_check_call(None, None)
    m._pag_begin()
    assert m.unet.calls == [(1 << 6) | (0b111 << 7)]
    m._pag_call = m._pag_check_call(0, None)
    m._pag_begin()
    assert m.unet.calls[-1] == 0 and len(m.unet.calls) == 2           # ... and one that had is switched off
    m.enable_pag(pag_scale=0.0)
    assert m._pag_check_call(None, None) is None and m._pag_check_call(2.0, None) == (2.0, 0.0)


def test_the_experiment_refuses_bad_sweeps_by_name():
    from sonicdiffusionbayeslab_amd.config import _wrap
    from sonicdiffusionbayeslab_amd.experiments.pag import PAGMethod
    m = PAGMethod.__new__(PAGMethod)
    m.config = _wrap({"model": {}, "experiment_params": {"pag_scale": [None, 3.0, 1.5], "pag_adaptive_scale": 0.01,
                                                        "pag_applied_layers": ["mid", "up.block_1"], "height": 512, "width": 768,
                                                        "num_inference_steps": [50]}})
    m.setup_exp_params()
    assert m.pag_scale == [None, 3.0, 1.5] and m.pag_adaptive_scale == 0.01 and m.pag_applied_layers == ["mid", "up.block_1"]
    assert m.size_kwargs == dict(height=512, width=768)
    for bad, match in (({"pag_scale": 3.0}, "list"), ({"pag_scale": ["3"]}, "pag_scale"),
                       ({"pag_scale": [3.0], "pag_adaptive_scale": -1}, "pag_adaptive_scale")):
        m.config = _wrap({"model": {}, "experiment_params": {"num_inference_steps": [50], **bad}})
        with pytest.raises(ValueError, match=match):
            m.setup_exp_params()


# ------------------------------------------------------------------------------------------------------------- the C ABI
def test_symbols_are_exported_and_the_abi_version_stays():
    lib = _lib.load()
    for s in NEW_SYMBOLS:
        assert s in _lib._SIGS and hasattr(lib, s), s
    assert lib.sd_abi_version() == 3


def test_sd_pag_identity_check_refuses_bad_shapes_without_a_gpu():
    lib = _lib.load()
    # (rows_total, row0, rows, C, heads, ldv, tok)
    ok = [(12, 8, 4, 1280, 8, 3840, 0), (384, 256, 128, 640, 8, 1920, 0), (768, 512, 256, 320, 8, 960, 0), (768, 512, 256, 320, 5, 960, 0),
          (768, 512, 256, 320, 8, 0, 256), (6144, 4096, 2048, 320, 8, 0, 1024), (6144, 4096, 2048, 320, 8, 0, 256),
          (1 << 31, 0, 1 << 31, 8, 1, 1 << 30, 0), (4, 3, 1, 320, 8, 320, 0)]
    for a in ok:
        assert lib.sd_pag_identity_check(*a) == 0, (a, lib.sd_last_error())
    bad = [((0, 0, 1, 320, 8, 960, 0), "rows"), (((1 << 31) + 1, 0, 1, 320, 8, 960, 0), "rows"),
           ((12, 8, 5, 320, 8, 960, 0), "rows ["), ((12, -1, 4, 320, 8, 960, 0), "rows ["), ((12, 8, 0, 320, 8, 960, 0), "rows ["),
           ((12, 8, 4, 324, 8, 972, 0), "C="), ((12, 8, 4, 320, 0, 960, 0), "C="), ((12, 8, 4, 320, 3, 960, 0), "C="),
           ((12, 8, 4, 16392, 1, 3 * 16392, 0), "C="), ((12, 8, 4, 320, 80, 960, 0), "C="),
           ((12, 8, 4, 320, 8, 312, 0), "pitch"), ((12, 8, 4, 320, 8, 324, 0), "pitch"), ((12, 8, 4, 320, 8, (1 << 30) + 8, 0), "pitch"),
           ((12, 8, 4, 320, 8, 960, -1), "pitch"),
           ((768, 512, 256, 320, 8, 0, 200), "head-major"), ((768, 500, 256, 320, 8, 0, 256), "head-major"),
           ((768, 512, 128, 320, 8, 0, 256), "head-major")]
    for a, what in bad:
        assert lib.sd_pag_identity_check(*a) == -1, a
        msg = lib.sd_last_error().decode()
        assert msg.startswith("sd_pag_identity_check:") and what in msg, (a, msg)


# ------------------------------------------------------------------------------------------------------------ the oracle
def test_oracle_with_no_layer_named_is_the_plain_oracle_and_the_unperturbed_samples_are_untouched():
    from oracle.unet import unet_forward
    case = po.UNET_CASES[0]
    name, h, w, lb, seed, t, layers, n = case
    cfg, sd, ocfg, heads = po.env(name)
    lat, ctx, sample = po.unet_inputs(cfg, h, w, lb, 3, seed)
    with torch.no_grad():
        plain = unet_forward(sd, ocfg, sample, t, ctx)
        off = po.unet_forward(sd, ocfg, sample, t, ctx, po.PagRun(ocfg, lb, 3 * lb, ()))
    assert torch.equal(off, plain)
    ref = po.reference(case)
    # every op but attention is per sample: the unperturbed samples of a PAG forward are those of the plain forward (up to the
    # batch size's effect on fp32 summation order in the CPU kernels)
    assert torch.allclose(ref["eps"][:2 * lb], plain[:2 * lb], rtol=0, atol=1e-4 * float(plain.abs().max()))
    # the perturbed third's prompt rows are the cond third's, so the two differ by the perturbation alone
    assert torch.equal(ctx[lb:2 * lb], ctx[2 * lb:]) and torch.equal(sample[lb:2 * lb], sample[2 * lb:])
    # both batch forms share the latents and the positive prompt
    lat2, ctx2, sample2 = po.unet_inputs(cfg, h, w, lb, 2, seed)
    assert torch.equal(lat2, lat) and torch.equal(ctx2[:lb], ctx[lb:2 * lb]) and ctx2.shape[0] == sample2.shape[0] == 2 * lb


def test_identity_attention_by_hand():
    """attn1 of a perturbed sample is to_out(to_v(x)) row by row: it does not see the other tokens."""
    import oracle.unet as ou
    g = torch.Generator().manual_seed(3)
    c, heads, p = 16, 2, "b.transformer_blocks.0.attn1."
    p2 = "b.transformer_blocks.0.attn2."
    w = {q + k: torch.randn(c, c, generator=g) for q in (p, p2) for k in ("to_q.weight", "to_k.weight", "to_v.weight", "to_out.0.weight")}
    w[p + "to_out.0.bias"], w[p2 + "to_out.0.bias"] = torch.randn(c, generator=g), torch.randn(c, generator=g)
    x = torch.randn(3, 5, c, generator=g)
    cfg = po.env("sd15")[2]
    run = po.PagRun(cfg, 1, 3, ())
    run.prefixes = {"b."}
    with po.patched(run):
        y = ou._attention(w, p, x, x, heads)
        other = ou._attention(w, p2, x, x, heads)
    plain = ou._attention(w, p, x, x, heads)
    assert torch.equal(y[:2], ou._attention(w, p, x[:2], x[:2], heads)) and run.used == ["b."]
    assert torch.equal(other, ou._attention(w, p2, x, x, heads))       # attn2 of the same block is untouched
    want = (x[2] @ w[p + "to_v.weight"].T) @ w[p + "to_out.0.weight"].T + w[p + "to_out.0.bias"]
    assert torch.allclose(y[2], want, atol=1e-5) and not torch.allclose(y[2], plain[2], atol=1e-2)
    x2 = x.clone()
    x2[2, 1:] = 0.0                                                   # other tokens of the perturbed sample do not reach token 0
    with po.patched(run):
        assert torch.equal(ou._attention(w, p, x2, x2, heads)[2, 0], y[2, 0])
    assert ou._attention is not None and "attention" not in po._ORIG  # the patch is gone


_ALL = [(c, rep, 0) for c in po.UNET_CASES for rep in (3, 2)] + [(po.SD2_CASE, 3, 0), (po.HT_CASE, 3, po.HT_TOKENS), (po.HM_CASE, 3, 0)]


@pytest.mark.parametrize("case,rep,tile", _ALL, ids=lambda v: f"{v[0]}-lb{v[3]}-" + "+".join(v[6]) if isinstance(v, tuple) else str(v))
def test_oracle_perturbed_against_cond_distance_at_every_unet_case_of_the_gpu_tests(case, rep, tile):
    """With the oracle alone, at the GPU test's inputs and against the floor the GPU test uses, 5 x UNET_TOL = 0.10.  Measured
    (the same at 3 and at 2 copies): sd15 16x16 mid + up.block_1 0.144, + down.block_2 0.199, down.block_0.attentions_0 0.906,
    down.block_0 1.014; two_level 32x32 down.block_0 + up.block_1 1.011 (2 latents) and 1.076 (3); sd2 0.582; with HyperTile 0.396.  ``mid`` alone gives
    0.025, below the floor: it is tested at the "mid" debug tensor (next test)."""
    from tests.util import rel_l2
    name, h, w, lb, seed, t, layers, n = case
    ref = po.reference(case, rep, tile)
    ocfg = po.env(name)[2]
    assert len(ref["used"]) == n and ref["used"] == [po.block_prefixes(ocfg)[k][1] for k in po.layer_bits(ocfg, layers)]
    eps = ref["eps"]
    d = rel_l2(eps[-lb:], eps[-2 * lb:-lb])
    print(f"oracle perturbed / cond, {name} {h}x{w} lb {lb} x{rep} {layers} tile {tile}: {d:.3f} (floor {po.FLOOR})")
    assert po.FLOOR == 5 * 2e-2 and d > po.FLOOR, d
    # the unperturbed samples are those of the plain forward at (rep - 1) * lb
    assert rel_l2(eps[:-lb], ref["plain"]) < 1e-4


def test_oracle_distance_of_the_default_layer_set_at_the_mid_tensor():
    """``pag_applied_layers="mid"`` moves the UNet output by 0.025 at this shape, below the floor, so the GPU test compares the
    "mid" debug tensor, where the oracle's own perturbed-against-cond distance is 0.30 (floor 0.10)."""
    from tests.util import rel_l2
    name, h, w, lb, seed, t, layers, n = po.MID_CASE
    ref = po.reference(po.MID_CASE)
    assert ref["used"] == ["mid_block.attentions.0."]
    mid = ref["mid"]
    d, d_out = rel_l2(mid[-lb:], mid[-2 * lb:-lb]), rel_l2(ref["eps"][-lb:], ref["eps"][-2 * lb:-lb])
    print(f"oracle perturbed / cond with 'mid': mid tensor {d:.3f} (floor {po.MID_FLOOR}), output {d_out:.3f}")
    assert po.MID_FLOOR == 5 * 2e-2 and d > po.MID_FLOOR and d_out < po.FLOOR
    assert rel_l2(mid[:-lb], ref["mid_plain"]) < 1e-4
