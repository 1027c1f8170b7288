"""FreeU without a GPU: the oracle (tests/freeu_oracle.py) -- FFT form against the closed form the kernel evaluates, the
identity, the asymmetric box -- its with / without distance at every UNet case of the GPU tests, the registry key and YAML keys,
every refusal by name, and the exported symbols."""
import math
import os

import pytest
import torch

from sonicdiffusionbayeslab_amd import _lib
from tests import freeu_oracle as fo

NEW_SYMBOLS = ["sd_unet_set_freeu", "sd_unet_disable_freeu", "sd_op_freeu"]


# ---------------------------------------------------------------------------------------------------------------- oracle
@pytest.mark.parametrize("H,W", fo.PLANES)
@pytest.mark.parametrize("s", [0.9, 0.2, 1.7])
def test_fft_form_equals_the_closed_form(H, W, s):
    x = torch.randn(2, 3, H, W, generator=torch.Generator().manual_seed(H * 100 + W))
    got, want = fo.fourier_filter(x, 1, s), fo.fourier_filter_closed(x, s)
    d = (got.double() - want).abs().max().item()
    print(f"fft vs closed form at {H}x{W}, s={s}: {d:.2e}")
    assert d < 1e-5, d
    assert (fo.fourier_filter(x.double(), 1, s) - want).abs().max().item() < 1e-12       # (fp64 FFT: the form is exact)


def test_s1_b1_is_the_identity_and_nothing_is_mutated():
    g = torch.Generator().manual_seed(1)
    h, k = torch.randn(2, 64, 5, 7, generator=g), torch.randn(2, 32, 5, 7, generator=g)
    h0, k0 = h.clone(), k.clone()
    for block in (0, 1):
        hh, kk = fo.apply_freeu(block, h, k, 1.0, 1.0, 1.0, 1.0)
        assert torch.equal(hh, h) and (kk - k).abs().max().item() < 1e-6
    hh, kk = fo.apply_freeu(0, h, k, 0.5, 9.0, 1.5, 9.0)           # block 0 reads (b1, s1)
    assert torch.equal(hh[:, :32], h[:, :32] * 1.5) and torch.equal(hh[:, 32:], h[:, 32:])
    assert torch.allclose(kk, fo.fourier_filter(k, 1, 0.5))
    hh, kk = fo.apply_freeu(1, h, k, 9.0, 0.5, 9.0, 1.5)           # block 1 reads (b2, s2)
    assert torch.equal(hh[:, :32], h[:, :32] * 1.5) and torch.allclose(kk, fo.fourier_filter(k, 1, 0.5))
    hh, kk = fo.apply_freeu(2, h, k, 0.5, 0.5, 1.5, 1.5)           # the other up blocks are untouched
    assert hh is h and kk is k
    assert torch.equal(h, h0) and torch.equal(k, k0)


@pytest.mark.parametrize("H,W", [(4, 4), (5, 7), (8, 12)])
def test_the_box_is_asymmetric(H, W):
    """A constant comes out times s; cos(2 pi n1 / H) times (1 + s) / 2 (only its -1 half is in the box);
    cos(2 pi (n1 / H - n2 / W)) unchanged ((-1, +1) and (+1, -1) are outside); cos(2 pi (n1 / H + n2 / W)) times (1 + s) / 2."""
    s = 0.2
    n1 = torch.arange(H, dtype=torch.float64)[:, None].expand(H, W)
    n2 = torch.arange(W, dtype=torch.float64)[None, :].expand(H, W)
    for form in (lambda x: fo.fourier_filter(x, 1, s), lambda x: fo.fourier_filter_closed(x, s)):
        const = torch.full((1, 1, H, W), 3.0, dtype=torch.float64)
        assert torch.allclose(form(const), s * const, atol=1e-12)
        c10 = torch.cos(2 * math.pi * n1 / H)[None, None]
        assert torch.allclose(form(c10), (1 + s) / 2 * c10, atol=1e-12)
        anti = torch.cos(2 * math.pi * (n1 / H - n2 / W))[None, None]
        assert torch.allclose(form(anti), anti, atol=1e-12)
        diag = torch.cos(2 * math.pi * (n1 / H + n2 / W))[None, None]
        assert torch.allclose(form(diag), (1 + s) / 2 * diag, atol=1e-12)


def test_hidden_channel_counts_of_the_up_resnets():
    cfg, sd, ocfg, _ = fo.env("sd15")
    assert [fo.hidden_channels(sd, f"up_blocks.0.resnets.{j}.") for j in range(3)] == [1280, 1280, 1280]
    assert [fo.hidden_channels(sd, f"up_blocks.1.resnets.{j}.") for j in range(3)] == [1280, 1280, 1280]
    assert [fo.hidden_channels(sd, f"up_blocks.2.resnets.{j}.") for j in range(3)] == [1280, 640, 640]


@pytest.mark.parametrize("case", fo.UNET_CASES, ids=[c[0] for c in fo.UNET_CASES])
def test_oracle_with_without_distance_at_every_unet_case_of_the_gpu_tests(case):
    """The distance the GPU test relies on, checked with the oracle alone at the GPU test's inputs.  Floors: 10 x UNET_TOL for
    the four-factor setting, 5 x UNET_TOL for every single-factor case (s1 = 0.9 alone moves eps by only 0.03 .. 0.04, so the case
    that proves block 0's filter is wired uses s1 = 0.2)."""
    from tests.util import rel_l2
    _, name, h, w, lb, ub, factors, floor = case
    plain, on = fo.reference(name, h, w, lb, ub, None), fo.reference(name, h, w, lb, ub, factors)
    d = rel_l2(on, plain)
    print(f"oracle with / without FreeU {factors}, {name} {h}x{w} batch {lb}/{ub}: {d:.3f} (floor {floor * fo.UNET_TOL})")
    assert d > floor * fo.UNET_TOL, d


@pytest.mark.parametrize("name", ["sd15", "sd2"])
def test_the_hook_reaches_the_six_resnets_in_order_and_off_is_the_plain_oracle(name):
    cfg, sd, ocfg, heads = fo.env(name)
    _, ctx, sample = fo.unet_inputs(cfg, 16, 16, 2, 2)
    calls = []
    on = fo.unet_forward(sd, ocfg, sample, fo.T_STEP, ctx, fo.GIVEN, heads_per_level=heads, calls=calls)
    assert calls == [f"up_blocks.{i}.resnets.{j}." for i in (0, 1) for j in range(3)]
    assert torch.equal(on, fo.reference(name, 16, 16, 2, 2, fo.GIVEN))                    # deterministic; nothing stays patched
    ones = fo.unet_forward(sd, ocfg, sample, fo.T_STEP, ctx, (1.0, 1.0, 1.0, 1.0), heads_per_level=heads)
    from tests.util import rel_l2
    # s = b = 1: the plain oracle up to the fp32 FFT round trip of the six skips (1e-6 per plane, fp32 layers behind it)
    assert rel_l2(ones, fo.reference(name, 16, 16, 2, 2, None)) < 1e-4


def test_the_swapped_setting_is_far_from_the_given_one():
    from tests.util import rel_l2
    d = rel_l2(fo.reference("sd15", 16, 16, 2, 2, fo.SWAPPED), fo.reference("sd15", 16, 16, 2, 2, fo.GIVEN))
    print(f"oracle, FreeU {fo.GIVEN} against its blocks-swapped form: {d:.3f}")
    assert d > 10 * fo.UNET_TOL, d
    assert fo.UNET_TOL == 2e-2


def test_deepcache_applies_freeu_to_the_cached_feature_on_consumption():
    """Two skip steps in a row on the same inputs give the same eps (the cached feature is not scaled twice), and it differs
    from the skip step of the plain oracle on the same cache."""
    from oracle.unet import DeepCacheState
    from tests.util import rel_l2
    cfg, sd, ocfg, heads = fo.env("sd15")
    _, ctx, sample = fo.unet_inputs(cfg, 16, 16, 2, 2)
    out = {}
    for factors in (None, fo.GIVEN):
        dc = DeepCacheState(cache_interval=3, cache_branch_id=7)          # cache block id 2: the branch reaches into up block 1
        dc.enabled = True
        eps = []
        for step, t in enumerate((981.0, 961.0, 961.0)):
            dc.cur_timestep = step
            eps.append(fo.unet_forward(sd, ocfg, sample, t, ctx, factors, dc=dc))
        assert torch.equal(eps[1], eps[2])
        out[factors] = eps
    assert rel_l2(out[fo.GIVEN][1], out[None][1]) > 5 * fo.UNET_TOL


# ------------------------------------------------------------------------------------------------- registry, YAML, refusals
def test_registry_key_and_yaml_keys():
    from sonicdiffusionbayeslab_amd.config import _wrap, load_config
    from sonicdiffusionbayeslab_amd.experiments.base_experiment import BaseMethod
    from sonicdiffusionbayeslab_amd.registry import methods_registry
    assert "freeu" in methods_registry
    cfg = load_config(os.path.join(os.path.dirname(__file__), "..", "configs", "freeu_config.yaml"))
    assert cfg.experiment.method == "freeu"
    settings = list(cfg.experiment_params.freeu)
    assert settings[0] is None
    assert BaseMethod.parse_freeu(_wrap({"freeu": settings[1]})) == dict(s1=0.9, s2=0.2, b1=1.5, b2=1.6)
    from sonicdiffusionbayeslab_amd.experiments.freeu import FreeUMethod
    method = object.__new__(FreeUMethod)                          # the plugin's own parsing of the sweep, nothing else of it
    method.config = cfg
    method.setup_exp_params()
    assert method.freeu == [None, dict(s1=0.9, s2=0.2, b1=1.5, b2=1.6)] and list(method.num_inference_steps) == [10, 20, 50]
    assert BaseMethod.parse_freeu(_wrap({"model_name": "x"})) is None
    assert BaseMethod.parse_freeu(_wrap({"freeu": None})) is None
    with pytest.raises(ValueError, match="s1, s2, b1, b2"):
        BaseMethod.parse_freeu(_wrap({"freeu": {"s1": 0.9, "s2": 0.2, "b1": 1.5}}))
    with pytest.raises(ValueError, match="s1, s2, b1, b2"):
        BaseMethod.parse_freeu(_wrap({"freeu": {"s1": 0.9, "s2": 0.2, "b1": 1.5, "b2": 1.6, "b3": 1.0}}))
    with pytest.raises(ValueError, match="mapping"):
        BaseMethod.parse_freeu(_wrap({"freeu": [0.9, 0.2, 1.5, 1.6]}))
    with pytest.raises(ValueError, match="b2"):
        BaseMethod.parse_freeu(_wrap({"freeu": {"s1": 0.9, "s2": 0.2, "b1": 1.5, "b2": 0.0}}))
    with pytest.raises(NotImplementedError, match="fp8"):
        BaseMethod.parse_freeu(_wrap({"freeu": {"s1": 0.9, "s2": 0.2, "b1": 1.5, "b2": 1.6}}), "fp8")


def test_every_refusal_by_name_before_any_gpu_work():
    from sonicdiffusionbayeslab_amd.models import StableDiffusionModel as M
    m = M()
    ok = dict(s1=0.9, s2=0.2, b1=1.5, b2=1.6)
    for name in ok:
        for bad in (0, 0.0, -1.0, float("nan"), float("inf"), "1.0", True, None):
            with pytest.raises(ValueError, match=rf"{name}=.*> 0"):
                m.enable_freeu(**{**ok, name: bad})
    with pytest.raises(NotImplementedError, match="fp8"):
        M(weight_dtype="fp8").enable_freeu(**ok)
    assert m._freeu is None                                        # nothing above took effect
    assert m.enable_freeu(**ok) is m and m._freeu == (0.9, 0.2, 1.5, 1.6)
    assert m.disable_freeu() is m and m._freeu is None
    assert M(weight_dtype="fp8").disable_freeu()._freeu is None    # off is never refused
    for cls in ("stable_diffusion_model", "stable_diffusion_model_two_schedulers", "stable_diffusion_model_interliving_schedulers",
                "stable_diffusion_model_skip_timesteps"):
        from sonicdiffusionbayeslab_amd.registry import models_registry
        assert hasattr(models_registry[cls], "enable_freeu") and hasattr(models_registry[cls], "disable_freeu")


# --------------------------------------------------------------------------------------------------------------- the ABI
def test_symbols_are_exported_and_the_abi_version_stays():
    lib = _lib.load()
    for n in NEW_SYMBOLS:
        assert hasattr(lib, n), n
        assert n in _lib._SIGS and n in _lib.declared_symbols(), n
    assert lib.sd_abi_version() == 3


def test_library_refuses_bad_settings_and_shapes_without_a_gpu():
    import ctypes as C
    from sonicdiffusionbayeslab_amd.unet import _c_config
    from sonicdiffusionbayeslab_amd.weights import UNetConfig
    lib = _lib.load()
    h = C.c_void_p()
    cfg = _c_config(UNetConfig(sample_size=16))
    _lib.check(lib.sd_unet_create(C.byref(cfg), C.byref(h)), "sd_unet_create")
    try:
        assert lib.sd_unet_set_freeu(h, 0.9, 0.2, 1.5, 1.6) == 0 and lib.sd_unet_disable_freeu(h) == 0
        for bad in ((0.0, 0.2, 1.5, 1.6), (0.9, -0.2, 1.5, 1.6), (0.9, 0.2, float("nan"), 1.6), (0.9, 0.2, 1.5, float("inf"))):
            assert lib.sd_unet_set_freeu(h, *bad) != 0
            assert b"set_freeu" in lib.sd_last_error() and b"> 0" in lib.sd_last_error()
    finally:
        lib.sd_unet_destroy(h)
    fp8 = _c_config(UNetConfig(sample_size=16), "fp8")
    _lib.check(lib.sd_unet_create(C.byref(fp8), C.byref(h)), "sd_unet_create")
    try:
        assert lib.sd_unet_set_freeu(h, 0.9, 0.2, 1.5, 1.6) != 0 and b"fp8" in lib.sd_last_error()
        assert lib.sd_unet_disable_freeu(h) == 0
    finally:
        lib.sd_unet_destroy(h)
    # the kernel's entry point checks its shapes on the host, before any launch (the pointers are never read)
    p = (256, 512, 768, 1024)
    assert lib.sd_op_freeu(None, *p, 1, 8, 8, 48, 32, 1.2, 0.9) != 0 and b"C_hidden=48 (a multiple of 32)" in lib.sd_last_error()
    assert lib.sd_op_freeu(None, *p, 1, 8, 8, 64, 40, 1.2, 0.9) != 0 and b"C_skip=40 (a multiple of 32)" in lib.sd_last_error()
    assert lib.sd_op_freeu(None, *p, 1, 1, 8, 64, 32, 1.2, 0.9) != 0 and b"plane 1x8" in lib.sd_last_error()
    assert lib.sd_op_freeu(None, *p, 1, 8, 129, 64, 32, 1.2, 0.9) != 0 and b"plane 8x129" in lib.sd_last_error()
    assert lib.sd_op_freeu(None, *p, 1, 8, 8, 64, 32, 0.0, 0.9) != 0 and b"> 0" in lib.sd_last_error()
    assert lib.sd_op_freeu(None, 256, 512, 256, 1024, 1, 8, 8, 64, 32, 1.2, 0.9) != 0 and b"new tensors" in lib.sd_last_error()
