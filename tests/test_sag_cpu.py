"""Self-attention guidance without a GPU: the exported symbols, the shape rules, every refusal by name, the registry key and YAML
keys, ``sag_scale = 0`` as the plain call, the degrade coefficients, and the oracle (tests/sag_oracle.py): its blur against
``F.conv2d``, the masses' mean, the strict threshold, and -- with the oracle alone, at the inputs of the GPU file -- the band, the
caps on the tokens a mask comparison leaves out, and the floor on what one SAG step moves."""
import math
import os

import pytest
import torch
import torch.nn.functional as F

from sonicdiffusionbayeslab_amd import _lib
from tests import sag_oracle as so
from tests.util import rel_l2

NEW_SYMBOLS = ["sd_unet_set_sag", "sd_unet_set_sag_buffer", "sd_sag_mass_check", "sd_op_sag_attn_mass", "sd_op_sag_degrade",
               "sd_sched_step_sag", "sd_sched_step_pc_sag"]


# ------------------------------------------------------------------------------------------------------------- the C ABI
def test_symbols_are_exported_and_declared_and_the_abi_version_stays():
    lib = _lib.load()
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "sd_hip.h")).read()
    for s in NEW_SYMBOLS:
        assert s in _lib._SIGS and hasattr(lib, s), s
        assert f" {s}(" in header, f"{s} is not declared in include/sd_hip.h"
    assert "SD_GUIDE_CFG_SAG = 4, SD_GUIDE_SAG = 5" in header
    assert lib.sd_abi_version() == 3


def test_sd_sag_mass_check_refuses_bad_shapes_without_a_gpu():
    lib = _lib.load()
    # (B, heads, N, D, ld, head_major)
    ok = [(2, 8, 16, 160, 3840, 0), (2, 8, 20, 160, 3840, 0), (1, 8, 63, 160, 3840, 0), (1, 20, 144, 64, 3840, 0), (2, 8, 256, 80, 1920, 0),
          (3, 8, 256, 160, 3840, 0), (2, 8, 20, 160, 3904, 0), (16, 8, 64, 160, 2560, 0), (65535, 1, 16, 64, 128, 0)]
    for a in ok:
        assert lib.sd_sag_mass_check(*a) == 0, (a, lib.sd_last_error())
    bad = [((2, 8, 20, 160, 3840, 1), "head-major"), ((0, 8, 20, 160, 3840, 0), "batch"), ((65536, 8, 20, 160, 3840, 0), "batch"),
           ((2, 8, 15, 160, 3840, 0), "tokens"), ((2, 8, 257, 160, 3840, 0), "tokens"), ((2, 8, 1024, 40, 960, 0), "tokens"),
           ((2, 8, 64, 40, 960, 0), "head dim"), ((2, 8, 64, 128, 3072, 0), "head dim"), ((2, 0, 64, 160, 3840, 0), "heads"),
           ((2, 65, 64, 64, 3 * 65 * 64, 0), "heads"), ((2, 8, 64, 160, 2552, 0), "pitch"), ((2, 8, 64, 160, 3844, 0), "pitch"),
           ((2, 8, 64, 160, (1 << 30) + 8, 0), "pitch")]
    for a, what in bad:
        assert lib.sd_sag_mass_check(*a) == -1, a
        msg = lib.sd_last_error().decode()
        assert msg.startswith("sd_sag_mass_check:") and what in msg, (a, msg)


def test_mid_grid_rule():
    from sonicdiffusionbayeslab_amd.unet import HipUNet2DConditionModel as U
    from sonicdiffusionbayeslab_amd.weights import UNetConfig
    cfg = UNetConfig(sample_size=16)
    assert U.sag_mid_grid(cfg, 32, 32) == (4, 4) and U.sag_mid_grid(cfg, 32, 40) == (4, 5) and U.sag_mid_grid(cfg, 128, 64) == (16, 8)
    for h, w in ((16, 16), (24, 32), (32, 36), (136, 64)):
        with pytest.raises(ValueError, match="mid grid"):
            U.sag_mid_grid(cfg, h, w)
    with pytest.raises(ValueError, match="factor"):
        U.sag_mid_grid(UNetConfig(sample_size=32, block_out_channels=(320, 640), attn_levels=(True, True)), 32, 32)


def test_degrade_coefficients():
    from sonicdiffusionbayeslab_amd.schedulers import PRED_TYPE_IDS, sag_degrade_coef
    assert PRED_TYPE_IDS == so.PRED_IDS
    a = 0.2318
    g = torch.Generator().manual_seed(1)
    x, m = torch.randn(64, dtype=torch.float64, generator=g), torch.randn(64, dtype=torch.float64, generator=g)
    for pred in ("epsilon", "v_prediction", "sample"):
        c = sag_degrade_coef(pred, a)
        x0, eps = so.x0_eps(x, m, a, pred)
        assert torch.allclose(c[0] * x + c[1] * m, x0, atol=1e-12) and torch.allclose(c[2] * x + c[3] * m, eps, atol=1e-12)
        assert c[4] == math.sqrt(a) and c[5] == math.sqrt(1 - a)
        # add_noise(x0, eps) is x again: a mask of zeros degrades nothing
        assert torch.allclose(c[4] * x0 + c[5] * eps, x, atol=1e-12)
    with pytest.raises(NotImplementedError, match="prediction_type"):
        sag_degrade_coef("flow", a)


# ------------------------------------------------------------------------------------------------- registry, YAML, refusals
def test_registry_key_and_yaml_keys():
    from sonicdiffusionbayeslab_amd.config import _wrap, load_config
    from sonicdiffusionbayeslab_amd.experiments.base_experiment import BaseMethod
    from sonicdiffusionbayeslab_amd.registry import methods_registry
    assert "sag" in methods_registry
    cfg = load_config(os.path.join(os.path.dirname(__file__), "..", "configs", "sag_config.yaml"))
    assert cfg.experiment.method == "sag" and list(cfg.experiment_params.sag_scale) == [None, 0.75]
    assert list(cfg.experiment_params.num_inference_steps) == [50] and cfg.scheduler.scheduler_name == "ddim_scheduler"
    assert BaseMethod.parse_sag(_wrap({"model_name": "x"})) is None
    assert BaseMethod.parse_sag(_wrap({"sag": {}})) == dict(sag_scale=0.75)
    assert BaseMethod.parse_sag(_wrap({"sag": {"scale": 0.5}})) == dict(sag_scale=0.5)
    with pytest.raises(ValueError, match="mapping"):
        BaseMethod.parse_sag(_wrap({"sag": 0.75}))
    with pytest.raises(ValueError, match="key scale"):
        BaseMethod.parse_sag(_wrap({"sag": {"sag_scale": 0.75}}))
    with pytest.raises(ValueError, match="sag_scale"):
        BaseMethod.parse_sag(_wrap({"sag": {"scale": "1"}}))
    with pytest.raises(NotImplementedError, match="fp8"):
        BaseMethod.parse_sag(_wrap({"sag": {"scale": 0.75}}), "fp8")


def test_the_experiment_sweeps_and_refuses_bad_sweeps_by_name():
    from sonicdiffusionbayeslab_amd.config import _wrap
    from sonicdiffusionbayeslab_amd.experiments.sag import SAGMethod
    m = SAGMethod.__new__(SAGMethod)
    m.config = _wrap({"model": {}, "experiment_params": {"sag_scale": [None, 0.75, 1.0], "height": 512, "width": 768,
                                                        "num_inference_steps": [20, 50]}})
    m.setup_exp_params()
    assert m.sag_scale == [None, 0.75, 1.0] and m.size_kwargs == dict(height=512, width=768)

    class Model:
        def __init__(self):
            self.log, self.scale = [], None

        def enable_sag(self, sag_scale):
            self.scale = sag_scale

        def disable_sag(self):
            self.scale = None
    m.model = Model()
    m.sweep = lambda steps, kw, title, extra: m.model.log.extend((m.model.scale, n, extra(n)["SAG"]) for n in steps)
    m.run_experiment()
    assert m.model.log == [(None, 20, "off"), (None, 50, "off"), (0.75, 20, "scale 0.75"), (0.75, 50, "scale 0.75"),
                           (1.0, 20, "scale 1.0"), (1.0, 50, "scale 1.0")] and m.model.scale is None
    for bad, match in (({"sag_scale": 0.75}, "list"), ({"sag_scale": ["1"]}, "sag_scale"), ({"sag_scale": [float("nan")]}, "sag_scale")):
        m.config = _wrap({"model": {}, "experiment_params": {"num_inference_steps": [50], **bad}})
        with pytest.raises(ValueError, match=match):
            m.setup_exp_params()


def test_every_refusal_by_name_before_any_gpu_work():
    import dataclasses
    from sonicdiffusionbayeslab_amd.models import (StableDiffusionModel as M, StableDiffusionModelInterlivingSchedulers,
                                                   StableDiffusionModelSkipTimesteps, StableDiffusionModelTwoSchedulers)
    from sonicdiffusionbayeslab_amd.weights import UNetConfig
    m = M()
    for bad in ("1", None, True, float("nan"), float("inf"), float("-inf")):
        with pytest.raises(ValueError, match="sag_scale"):
            m.enable_sag(sag_scale=bad)
    with pytest.raises(NotImplementedError, match="fp8"):
        M(weight_dtype="fp8").enable_sag()
    with pytest.raises(NotImplementedError, match="9-channel"):
        M(unet_config=dataclasses.replace(UNetConfig(sample_size=16), in_channels=9)).enable_sag()
    assert m._sag is None                                            # nothing above took effect
    for V in (StableDiffusionModelTwoSchedulers, StableDiffusionModelInterlivingSchedulers, StableDiffusionModelSkipTimesteps):
        with pytest.raises(NotImplementedError, match="variant pipelines"):
            V().enable_sag()
        with pytest.raises(NotImplementedError, match="variant pipelines"):
            V().call(prompt="a", sag_scale=0.75)
    # the call's own kwarg without enable_sag
    with pytest.raises(ValueError, match="enable_sag"):
        m._sag_check_call(0.75)
    assert m._sag_check_call(None) is None
    assert m.enable_sag() is m and m._sag == 0.75
    assert m._sag_check_call(None) == 0.75 and m._sag_check_call(0.5) == 0.5 and m._sag_check_call(1) == 1.0
    for bad in ("1", float("nan"), float("inf")):
        with pytest.raises(ValueError, match="sag_scale"):
            m._sag_check_call(bad)
    # what a SAG call refuses: PAG, guidance_rescale, Token Merging, T-GATE, DeepCache, IP-Adapter, ControlNet, a tiled mid block
    m._pag_call = (3.0, 0.0)
    with pytest.raises(NotImplementedError, match="PAG"):
        m._sag_check_call(None)
    m._pag_call = None
    with pytest.raises(NotImplementedError, match="guidance_rescale"):
        m._sag_check_call(None, guidance_rescale=0.7)
    m.apply_tome(ratio=0.5)
    with pytest.raises(NotImplementedError, match="Token Merging"):
        m._sag_check_call(None)
    m.remove_tome()
    m.enable_tgate(2)
    with pytest.raises(NotImplementedError, match="T-GATE"):
        m._sag_check_call(None)
    m.disable_tgate()
    m._deepcache = object()
    with pytest.raises(NotImplementedError, match="DeepCache"):
        m._sag_check_call(None)
    m._deepcache = None
    with pytest.raises(NotImplementedError, match="ControlNet"):
        m._sag_check_call(None, control=torch.zeros(1, 3, 8, 8))
    with pytest.raises(NotImplementedError, match="IP-Adapter"):
        m._sag_check_call(None, ip_adapter_image_embeds=torch.zeros(1, 8))
    with pytest.raises(NotImplementedError, match="IP-Adapter"):
        m._sag_check_call(None, ip_adapter_image=torch.zeros(1, 3, 8, 8))
    m.enable_hypertile(tile_size=64, max_depth=3)
    with pytest.raises(NotImplementedError, match="tiles the mid block"):
        m._sag_check_call(None)
    m.enable_hypertile(tile_size=64, max_depth=2)
    assert m._sag_check_call(None) == 0.75                           # HyperTile above the mid block composes
    m.disable_hypertile()
    # ... and none of them refuses a call whose scale is 0: that is the plain pipeline
    m.apply_tome(ratio=0.5)
    assert m._sag_check_call(0.0, guidance_rescale=0.7) is None
    m.remove_tome()
    assert m.disable_sag() is m and m._sag is None


def test_sag_scale_zero_leaves_the_unet_handle_alone():
    """``sag_scale <= 0`` (the default's or the call's) is a plain call: no capture on the UNet handle -- so the plan key is the
    plain one -- no second context and no ``sag_scale`` in the step."""
    from sonicdiffusionbayeslab_amd.models import StableDiffusionModel as M

    class Unet:
        _sag, _sag_mass, device = False, None, "cpu"

        def __init__(self):
            self.calls = []

        @staticmethod
        def sag_mid_grid(config, h, w):
            return h // 8, w // 8

        def set_sag(self, on, mass=None):
            self.calls.append(("set", on, None if mass is None else tuple(mass.shape)))
            self._sag = on
            self._sag_mass = mass if mass is not None else self._sag_mass

        def clear_sag(self):
            self.calls.append(("clear",))
            self._sag, self._sag_mass = False, None

        def set_sag_context(self, ctx, h, w):
            self.calls.append(("ctx", tuple(ctx.shape[:1]), h, w))
    m = M().enable_sag()
    m.unet = Unet()
    m._size = (256, 320)
    ctx = torch.zeros(4, 77, 768)
    for scale in (0.0, -1.0):
        m._sag_call = m._sag_check_call(scale)
        assert m._sag_call is None
        m._sag_begin(2, ctx)
        m._sag_context(2, ctx)
        assert m.unet.calls == []                                    # a handle that never had it is not touched
    m._sag_call = m._sag_check_call(None)
    m._sag_begin(2, ctx)
    m._sag_context(2, ctx)
    assert m.unet.calls == [("set", True, (4, 4 * 5)), ("ctx", (2,), 32, 40)]
    m._sag_call = m._sag_check_call(0)
    m._sag_begin(2, ctx)
    assert m.unet.calls[-1] == ("clear",) and len(m.unet.calls) == 3  # ... and one that had is switched off


# ------------------------------------------------------------------------------------------------------------ the oracle
def test_oracle_blur_is_the_reflect_padded_gaussian_convolution():
    g = torch.Generator().manual_seed(5)
    w = so.gauss_weights()
    assert w.shape == (9,) and abs(float(w.sum()) - 1.0) < 1e-15 and torch.equal(w, w.flip(0))
    assert abs(float(w[4] / w[3]) - math.exp(0.5)) < 1e-12            # exp(-0.5 i^2): sigma 1
    k2 = torch.outer(w, w)[None, None].repeat(4, 1, 1, 1)
    for shape in ((2, 4, 32, 32), (1, 4, 32, 40), (1, 4, 96, 96)):
        x = torch.randn(shape, dtype=torch.float64, generator=g)
        ref = F.conv2d(F.pad(x, (4, 4, 4, 4), mode="reflect"), k2, groups=4)
        assert float((so.blur(x) - ref).abs().max()) < 1e-13
    one = torch.ones(1, 4, 32, 32, dtype=torch.float64)
    assert float((so.blur(one) - one).abs().max()) < 1e-14            # normalised, also at the reflected edges


def test_mask_is_strict_at_exactly_one_and_upsamples_by_eight():
    m = torch.tensor([[1.0, 1.0 + 2.0 ** -23, 1.0 - 2.0 ** -24, 2.0]])
    assert so.mask_of(m).tolist() == [[False, True, False, True]]
    grid = torch.tensor([[[True, False], [False, True]]])
    up = so.upsample8(grid)
    assert up.shape == (1, 1, 16, 16)
    for y in range(16):
        for x in range(16):
            assert bool(up[0, 0, y, x]) == bool(grid[0, y // 8, x // 8])
    # a mask of zeros degrades nothing, a mask of ones blurs everything
    g = torch.Generator().manual_seed(7)
    x, mo = torch.randn(1, 4, 32, 32, dtype=torch.float64, generator=g), torch.randn(1, 4, 32, 32, dtype=torch.float64, generator=g)
    for pred in ("epsilon", "v_prediction", "sample"):
        assert torch.allclose(so.degrade(x, mo, 0.3, pred, torch.zeros(1, 4, 4, dtype=torch.bool)), x, atol=1e-12)
        full = so.degrade(x, mo, 0.3, pred, torch.ones(1, 4, 4, dtype=torch.bool))
        x0, eps = so.x0_eps(x, mo, 0.3, pred)
        assert torch.allclose(full, math.sqrt(0.3) * so.blur(x0) + math.sqrt(0.7) * eps, atol=1e-12)


def test_combine_by_hand():
    u, c, d = torch.tensor([1.0]), torch.tensor([3.0]), torch.tensor([0.5])
    assert so.combine(torch.cat([u, c]), d, 1, True, 7.5, 0.75).item() == (1.0 + 7.5 * 2.0) + 0.75 * 0.5
    assert so.combine(c, d, 1, False, 1.0, 0.75).item() == 3.0 + 0.75 * 2.5
    assert so.combine(torch.cat([u, c]), d, 1, True, 7.5, 0.0).item() == so.plain_guided(torch.cat([u, c]), 1, True, 7.5).item()


@pytest.mark.parametrize("case", so.UNET_CASES, ids=[f"{c[0]}-{c[1]}x{c[2]}" for c in so.UNET_CASES])
def test_oracle_mass_band_and_cap_at_every_unet_case_of_the_gpu_tests(case):
    """With the oracle alone, at the GPU test's inputs: the masses of a sample average 1, capture leaves the forward alone, the
    band (1.5 x the shift under noise of rel-L2 UNET_TOL on the attn1 input) and the share of tokens inside it against the
    cap.  Measured: sd15 32x32 shift 0.017 band 0.025 share 0.16; sd15 32x40 0.014 / 0.022 / 0.05; sd2 32x32 0.008 / 0.013 / 0.00;
    two_level 32x32 (256 tokens) 0.034 / 0.051 / 0.26."""
    name, h, w, lb, seed, t = case
    ref = so.reference(case)
    mass = ref["mass"]
    assert float((mass.double().mean(dim=1) - 1.0).abs().max()) < 1e-5
    share = float(((mass[:lb] - 1.0).abs() <= ref["band"]).float().mean())
    ones = float(so.mask_of(mass[:lb]).float().mean())
    print(f"oracle mass, {name} {h}x{w}: std {float(mass.std()):.3f} range {float(mass.min()):.2f} .. {float(mass.max()):.2f}; shift "
          f"{ref['shift']:.4f} band {ref['band']:.4f}; {share:.3f} of the tokens inside it (cap {so.MASK_CAP}); mask {ones:.2f} ones")
    assert so.BAND_FACTOR == 1.5 and so.MASK_CAP == 0.30 and ref["band"] == 1.5 * ref["shift"]
    assert 0.0 < ref["band"] < 0.06 and share <= so.MASK_CAP and 0.1 < ones < 0.9
    so.masks_agree(mass[:lb], so.mask_of(mass[:lb]), ref["band"], so.MASK_CAP, "the oracle against itself")


def test_oracle_capture_leaves_the_forward_alone_and_the_patch_goes():
    import oracle.unet as ou
    name, h, w, lb, seed, t = so.UNET_CASES[1]
    cfg, sd, ocfg, heads = so.env(name)
    lat, pe, ne = so.unet_inputs(cfg, h, w, lb, seed)
    with torch.no_grad():
        plain = ou.unet_forward(sd, ocfg, torch.cat([lat, lat]), t, torch.cat([ne, pe]))
    assert torch.equal(so.reference(so.UNET_CASES[1])["eps"], plain) and "attention" not in so._ORIG


@pytest.mark.parametrize("cfg_on", [False, True], ids=["nocfg", "cfg"])
def test_oracle_step_distance_and_cap_at_the_step_case(cfg_on):
    """One SAG step at s = 0.75 moves the guided prediction by 0.166 rel-L2 with CFG 7.5 (t = 981; 0.159 at t = 21 and 0.086 at
    t = 501, which is why that case is not there) and by 0.191 without CFG (t = 501, 0.094 of the tokens inside the band; at
    t = 981 it moves 0.312 but 0.344 of the tokens lie inside the band, above the cap).  The floor of the GPU test is 0.10."""
    case = so.STEP_CASES[cfg_on]
    lb = case[3]
    r = so.step_reference(case, cfg=cfg_on)
    moved = rel_l2(r["e"], r["plain"])
    print(f"oracle SAG step cfg={cfg_on}: e against the plain guided prediction {moved:.3f} (floor {so.MOVED_FLOOR}); |m - d| / |m| "
          f"{rel_l2(r['d'], r['eps1'][:lb]):.3f}; band {r['band']:.4f}")
    assert so.MOVED_FLOOR == 0.10 and moved >= so.MOVED_FLOOR
    if cfg_on:
        # what UNET_TOL per UNet output implies for e under CFG 7.5 (the GPU test's bound there), from the oracle alone: 0.156,
        # below what the step moves, so a prediction without the SAG term is still outside it for the oracle
        bound = so.cfg_step_bound(r, lb)
        print(f"oracle SAG step cfg: the bound UNET_TOL implies for e {bound:.4f}")
        assert 0.15 < bound < moved
    so.masks_agree(r["mass"], so.mask_of(r["mass"]), r["band"], so.MASK_CAP, "the step case")
    # forcing the oracle's own mask changes nothing; forcing its complement changes d
    same = so.step_reference(case, forced_mask=so.mask_of(r["mass"]), cfg=cfg_on)
    other = so.step_reference(case, forced_mask=~so.mask_of(r["mass"]), cfg=cfg_on)
    assert torch.equal(same["e"], r["e"]) and rel_l2(other["d"], r["d"]) > 0.05


@pytest.mark.parametrize("cfg_on", [True, False], ids=["cfg", "nocfg"])
def test_oracle_loop_distance_from_the_plain_loop(cfg_on):
    """The 3-step DDIM call of the GPU file at 256 px with the oracle alone: the SAG loop ends more than FREE_TOL from the plain
    loop, and every step's own mask meets the cap at that step's band."""
    from oracle.schedulers import DDIMOracle
    from sonicdiffusionbayeslab_amd.weights import UNetConfig, make_synthetic_state_dict
    from tests.util import oracle_cfg
    cfg = UNetConfig(sample_size=16)
    sd = make_synthetic_state_dict(cfg, seed=1234)
    g = torch.Generator().manual_seed(91)
    lat = torch.randn(1, 4, 32, 32, generator=g)
    pe, ne = (torch.randn(1, cfg.context_len, cfg.cross_attention_dim, generator=g) for _ in range(2))
    o = DDIMOracle()
    o.set_timesteps(3)
    step = lambda e, t, x: o.step(e, t, x, return_dict=False)[0]      # noqa: E731
    gs = so.GS if cfg_on else 1.0
    args = (sd, oracle_cfg(cfg), step, o.alphas_cumprod, "epsilon", o.timesteps, pe, ne if cfg_on else None, lat, gs)
    out, masses, bands = so.loop(*args, so.SAG_SCALE)
    plain, _, _ = so.loop(*args, 0.0)
    moved = rel_l2(out, plain)
    print(f"oracle loop cfg={cfg_on}: SAG against plain {moved:.3f} (FREE_TOL {so.FREE_TOL}); bands {[round(b, 4) for b in bands]}")
    assert moved > so.FREE_TOL
    for i, (m, b) in enumerate(zip(masses, bands)):
        so.masks_agree(m, so.mask_of(m), b, so.MASK_CAP, f"loop step {i}")


def test_oracle_distance_of_the_v_prediction_call_on_the_sd2_shaped_unet():
    """The GPU file's SD 2.x-shaped v-prediction call with the oracle alone: 0.073 from the plain loop without CFG (0.024 under
    CFG 7.5, below FREE_TOL: the GPU file runs this call without CFG)."""
    from sonicdiffusionbayeslab_amd.registry import schedulers_registry
    from sonicdiffusionbayeslab_amd.schedulers import PNDMConfigStub
    from tests import sched_ref as R
    cfg, sd, ocfg, heads = so.env("sd2")
    s = schedulers_registry["ddim_scheduler"].from_config(PNDMConfigStub().config, prediction_type="v_prediction")
    s.set_timesteps(3)
    g = torch.Generator().manual_seed(97)
    lat = torch.randn(1, 4, 32, 32, generator=g)
    pe = torch.randn(1, cfg.context_len, cfg.cross_attention_dim, generator=g)
    outs = []
    for scale in (so.SAG_SCALE, 0.0):
        rs = R.DDIM(torch.from_numpy(s.alphas_cumprod), s._timesteps_list, "v_prediction", s.final_alpha_cumprod)
        out, masses, bands = so.loop(sd, ocfg, lambda e, t, x: rs.step(e, t, x.double())[0], s.alphas_cumprod, "v_prediction",
                                     s._timesteps_list, pe, None, lat, 1.0, scale, heads_per_level=heads)
        outs.append(out)
        if scale:
            for i, (m, b) in enumerate(zip(masses, bands)):
                so.masks_agree(m, so.mask_of(m), b, so.MASK_CAP, f"sd2 loop step {i}")
    moved = rel_l2(outs[0], outs[1])
    print(f"oracle loop, SD 2.x-shaped, v-prediction, no CFG: SAG against plain {moved:.3f} (FREE_TOL {so.FREE_TOL})")
    assert moved > so.FREE_TOL


def test_the_step_refuses_guidance_rescale_and_pag_with_sag_before_any_launch():
    from sonicdiffusionbayeslab_amd.registry import schedulers_registry
    from sonicdiffusionbayeslab_amd.schedulers import PNDMConfigStub
    for name in ("ddim_scheduler", "dpm_solver_scheduler", "lcm_scheduler", "pndm_scheduler", "unipc_scheduler"):
        s = schedulers_registry[name].from_config(PNDMConfigStub().config)
        with pytest.raises(NotImplementedError, match="guidance_rescale"):
            s._rescale(None, True, 7.5, 0.7, None, None, 0.75)        # (raised before eps is touched)
        with pytest.raises(NotImplementedError, match="PAG and SAG"):
            s._rescale(None, True, 7.5, 0.0, None, 3.0, 0.75)
        assert s._rescale(None, True, 7.5, 0.0, None, None, 0.75) is None
        assert s._pag_kw(None, 0.75) == {"sag": 0.75} and s._pag_kw(3.0) == {"pag": 3.0} and s._pag_kw(None) == {}
