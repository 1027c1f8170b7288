"""The table of UNet option pairs that are not built (``options.py`` above the library, ``csrc/model.h`` inside it) and the
plan key, without a GPU: the two tables agree name by name and pair by pair; every refused pair is refused by a
``StableDiffusionModel`` before any handle exists, by the names of both, in either order; every pair of the six switchable
options that is NOT in the table goes through; and ``PlanVariant`` orders by every one of its fields (a stand-alone host program)."""
import ctypes as C
import dataclasses
import itertools

import pytest
import torch

from sonicdiffusionbayeslab_amd import _lib, options as O
from sonicdiffusionbayeslab_amd.models import (StableDiffusionModel, StableDiffusionModelInterlivingSchedulers,
                                               StableDiffusionModelSkipTimesteps, StableDiffusionModelTwoSchedulers)
from sonicdiffusionbayeslab_amd.unet import _c_config
from sonicdiffusionbayeslab_amd.weights import UNetConfig


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


# ------------------------------------------------------------------------------------------------ (a) the two tables agree
def _c_names(lib):
    names = []
    while lib.sd_unet_option_name(len(names)) is not None:
        names.append(lib.sd_unet_option_name(len(names)).decode())
        assert len(names) < 64
    return names


def test_the_library_and_python_name_the_same_options_in_the_same_order(lib):
    names = _c_names(lib)
    assert tuple(names) == O.HANDLE_OPTIONS
    assert lib.sd_unet_option_name(-1) is None and lib.sd_unet_option_name(len(names)) is None
    assert set(O.OPTIONS) - set(O.HANDLE_OPTIONS) == {O.VARIANT, O.RESCALE}      # the rows only a pipeline has


def test_the_library_and_python_refuse_the_same_pairs_for_the_same_reason(lib):
    names = _c_names(lib)
    refused = set()
    for a, b in itertools.product(range(len(names)), repeat=2):
        why = lib.sd_unet_option_conflict(a, b)
        why = None if why is None else why.decode()
        assert why == O.conflict(names[a], names[b]), (names[a], names[b])        # ... in both argument orders: the product has both
        if why is not None:
            refused.add(frozenset((names[a], names[b])))
    assert refused == {frozenset(k) for k in O.HANDLE_PAIRS} and len(refused) == len(O.HANDLE_PAIRS)
    assert all(len(p) == 2 for p in refused)                                      # no option is refused with itself
    for a, b in ((-1, 0), (0, -1), (len(names), 0), (0, len(names))):
        assert lib.sd_unet_option_conflict(a, b) is None
    # the pipeline rows name an option the library does not have
    assert all(a in (O.VARIANT, O.RESCALE) or b in (O.VARIANT, O.RESCALE) for a, b in O.PIPELINE_PAIRS)
    assert not set(map(frozenset, O.PIPELINE_PAIRS)) & set(map(frozenset, O.HANDLE_PAIRS))


def test_check_names_both_options_the_reason_and_the_way_out():
    with pytest.raises(NotImplementedError) as e:
        O.check(O.PAG, [O.FREEU, O.TOME])
    assert str(e.value) == "PAG with Token Merging is not built: merged tokens have no identity attention (remove_tome() first)"
    with pytest.raises(NotImplementedError, match=r"set_pag\(0\) first"):
        O.check(O.TOME, [O.PAG], O.HANDLE_OFF)
    O.check(O.PAG, [O.FREEU, O.HYPERTILE, O.PAG])
    O.check(O.FREEU, O.OPTIONS[3:])                     # (FreeU is refused on fp8 alone)
    assert O.conflict(O.PAG, O.TOME) == O.conflict(O.TOME, O.PAG) and O.conflict(O.PAG, O.PAG) is None


# ------------------------------------------------------------------------- (b), (c) the pipeline, before any handle exists
CFG = UNetConfig(sample_size=16)
VARIANTS = (StableDiffusionModelTwoSchedulers, StableDiffusionModelInterlivingSchedulers, StableDiffusionModelSkipTimesteps)

# how a model comes to have an option: by construction ...
BUILD = {O.FP8: lambda cls: cls(unet_config=CFG, state_dict={}, weight_dtype="fp8"),
         O.INPAINT9: lambda cls: cls(unet_config=dataclasses.replace(CFG, in_channels=9), state_dict={}),
         O.IP_MODEL: lambda cls: cls(unet_config=dataclasses.replace(CFG, ip_adapter_tokens=4, ip_adapter_embed_dim=1024), state_dict={})}
# ... through enable_* / apply_tome / the DeepCache helper ...
ENABLE = {O.TOME: lambda m: m.apply_tome(ratio=0.5), O.HYPERTILE: lambda m: m.enable_hypertile(tile_size=64),
          O.FREEU: lambda m: m.enable_freeu(0.9, 0.2, 1.5, 1.6), O.TGATE: lambda m: m.enable_tgate(2),
          O.PAG: lambda m: m.enable_pag(), O.SAG: lambda m: m.enable_sag(),
          O.DEEPCACHE: lambda m: setattr(m, "_deepcache", object())}
# ... or with an argument of the call
CALL = {O.CONTROL: dict(control=torch.zeros(1, 3, 8, 8)), O.IP_PROMPT: dict(ip=torch.zeros(1, 8)), O.RESCALE: dict(rescale=0.7)}


def _call_checks(m, control=None, ip=None, rescale=0.0):
    """The checks ``call`` makes before any GPU work, in its order."""
    m._pag_call = m._pag_check_call(None, None, control, None, ip)
    m._sag_call = m._sag_check_call(None, rescale, control, None, ip)
    m._tgate_check_call(control, None, ip)
    if control is not None:
        m._cn_cfg = object()                            # (a loaded ControlNet: the argument checks come after the pair's)
        m._control_args(control, 1.0, 0.0, 1.0, False, None, 1)


def _run(first, second, cls=StableDiffusionModel):
    """A model that takes on ``first``, then ``second``, then runs the call-time checks; it never builds a UNet handle."""
    m = BUILD[first](cls) if first in BUILD else cls(unet_config=CFG, state_dict={})
    kw = {}
    for o in (first, second):
        if o in ENABLE:
            ENABLE[o](m)
        elif o in CALL:
            kw.update(CALL[o])
    try:
        _call_checks(m, **kw)
    finally:
        assert m.unet is None
    return m


def _orders(a, b):
    """Both orders of taking the pair on, where both exist: a model is built with its properties before anything is enabled."""
    if O.VARIANT in (a, b):
        return []
    return [(a, b)] if a in BUILD else [(b, a)] if b in BUILD else [(a, b), (b, a)]


ALL_PAIRS = sorted({**O.HANDLE_PAIRS, **O.PIPELINE_PAIRS})


@pytest.mark.parametrize("a,b", ALL_PAIRS, ids=[f"{a} x {b}".replace(" ", "_") for a, b in ALL_PAIRS])
def test_every_pair_in_the_table_is_refused_by_name_before_any_handle_exists(a, b):
    if O.VARIANT in (a, b):
        other = b if a == O.VARIANT else a
        for V in VARIANTS:
            with pytest.raises(NotImplementedError) as e:
                ENABLE[other](V(unet_config=CFG, state_dict={}))
            assert "variant pipelines" in str(e.value) and other in str(e.value)
        return
    assert _orders(a, b)
    for first, second in _orders(a, b):
        with pytest.raises(NotImplementedError) as e:
            _run(first, second)
        assert a in str(e.value) and b in str(e.value), str(e.value)


SWITCHABLE = (O.TOME, O.HYPERTILE, O.FREEU, O.TGATE, O.PAG, O.SAG)
# written out, not computed from the table under test: the 15 pairs of the six less the six that are refused
ALLOWED = [(O.TOME, O.FREEU), (O.TOME, O.TGATE), (O.HYPERTILE, O.FREEU), (O.HYPERTILE, O.TGATE), (O.HYPERTILE, O.PAG),
           (O.HYPERTILE, O.SAG), (O.FREEU, O.TGATE), (O.FREEU, O.PAG), (O.FREEU, O.SAG)]


@pytest.mark.parametrize("a,b", ALLOWED, ids=[f"{a} x {b}".replace(" ", "_") for a, b in ALLOWED])
def test_every_pair_outside_the_table_goes_through(a, b):
    for first, second in ((a, b), (b, a)):
        m = _run(first, second)
        on = dict(zip(SWITCHABLE, (m._tome, m._hypertile, m._freeu, m._tgate_step, m._pag, m._sag)))
        assert on[a] is not None and on[b] is not None
        assert (m._pag_call is not None) == (O.PAG in (a, b)) and (m._sag_call is not None) == (O.SAG in (a, b))


def test_the_allowed_list_and_the_table_cover_the_six_switchable_options():
    refused = [p for p in itertools.combinations(SWITCHABLE, 2) if O.conflict(*p)]
    assert len(ALLOWED) == 9 and len(refused) == 6
    assert {frozenset(p) for p in ALLOWED} | {frozenset(p) for p in refused} == {frozenset(p) for p in itertools.combinations(SWITCHABLE, 2)}


def test_one_model_across_calls_sees_this_call_not_the_last_one():
    """A PAG call, then PAG off and T-GATE on: the second call runs, as it did before the table (and a call with the scale
    at 0 beside T-GATE too); with PAG still on it is refused."""
    m = StableDiffusionModel(unet_config=CFG, state_dict={})
    m.enable_pag()
    _call_checks(m)
    assert m._pag_call == (3.0, 0.0)
    m.disable_pag()
    m.enable_tgate(2)
    _call_checks(m)
    assert m._pag_call is None and m._sag_call is None
    m.enable_pag(pag_scale=0.0)                         # (PAG enabled at scale 0 is the plain pipeline)
    _call_checks(m)
    m.enable_pag()
    with pytest.raises(NotImplementedError, match="T-GATE"):
        _call_checks(m)
    m.disable_tgate()
    m.enable_sag()
    with pytest.raises(NotImplementedError, match="PAG"):
        _call_checks(m)
    m.disable_pag()
    _call_checks(m)
    assert m._pag_call is None and m._sag_call == 0.75 and m.unet is None


# ----------------------------------------------------------------------------------------------------- (d) the plan key
def test_plan_variant_orders_by_every_field_and_follows_the_handle_state(tmp_path):
    """tests/plan_variant_host.cpp, a stand-alone host program over csrc/model.h: flipping each of the sixteen fields in turn
    gives a distinct key, the fields compare in their order, two handles in equal state give equal keys."""
    import os
    import shutil
    import subprocess
    from sonicdiffusionbayeslab_amd.build import LIB_DIR
    here = os.path.dirname(os.path.abspath(__file__))
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    hipcc = hipcc if os.path.exists(hipcc) else shutil.which("hipcc")
    assert hipcc, "hipcc builds the library and this program"
    exe = str(tmp_path / "plan_variant_host")
    subprocess.run([hipcc, "-std=c++17", "-x", "hip", "--offload-arch=gfx950", "-O0", os.path.join(here, "plan_variant_host.cpp"),
                    "-L" + LIB_DIR, "-lsdhip", "-Wl,-rpath," + LIB_DIR, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert (r.returncode, r.stdout.strip()) == (0, "ok"), r.stdout + r.stderr


def test_the_library_setters_share_the_table(lib):
    """Token Merging beside PAG is refused by ``sd_unet_set_tome`` itself, by the names of both (before the table only the
    wrapper refused it), and nothing takes effect."""
    h = C.c_void_p()
    cc = _c_config(CFG)
    _lib.check(lib.sd_unet_create(C.byref(cc), C.byref(h)), "sd_unet_create")
    try:
        _lib.check(lib.sd_unet_set_pag(h, 1 << 6), "sd_unet_set_pag")
        assert lib.sd_unet_set_tome(h, 0.5, 1) != 0
        err = lib.sd_last_error().decode()
        assert "set_tome" in err and "Token Merging" in err and "PAG" in err
        _lib.check(lib.sd_unet_set_pag(h, 0), "sd_unet_set_pag")
        _lib.check(lib.sd_unet_set_tome(h, 0.5, 1), "sd_unet_set_tome")
        assert lib.sd_unet_set_sag(h, 1) != 0 and "SAG" in lib.sd_last_error().decode()
    finally:
        lib.sd_unet_destroy(h)
