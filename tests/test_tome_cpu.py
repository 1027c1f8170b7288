"""Token Merging without a GPU: the oracle (tests/tome_oracle.py) on a 4x4 grid worked by hand, its with / without distance at
every UNet case of the GPU tests, the registry key and YAML keys, every refusal by name, the dst-choice draw, and the exported
symbols."""
import pytest
import torch

from sonicdiffusionbayeslab_amd import _lib
from tests import tome_oracle as to

NEW_SYMBOLS = ["sd_unet_set_tome", "sd_unet_set_tome_choice_hw", "sd_unet_tome_block_count_hw", "sd_unet_tome_block_info_hw",
               "sd_unet_tome_matching_hw", "sd_op_tome_match", "sd_op_tome_select", "sd_op_tome_merge", "sd_op_tome_unmerge"]


# ---------------------------------------------------------------------------------------------------------------- oracle
def test_partition_of_a_4x4_grid_by_hand():
    # cells (row-major): choice 0 -> token (0,0); 1 -> (0,3); 2 -> (3,0); 3 -> (3,3)
    src, dst = to.partition(torch.tensor([0, 1, 2, 3], dtype=torch.uint8), 4, 4)
    assert dst.tolist() == [0, 3, 12, 15]
    assert src.tolist() == [1, 2, 4, 5, 6, 7, 8, 9, 10, 11, 13, 14]
    src0, dst0 = to.partition(torch.zeros(4, dtype=torch.uint8), 4, 4)        # use_rand=False: the top-left token of every cell
    assert dst0.tolist() == [0, 2, 8, 10] and src0.tolist() == [1, 3, 4, 5, 6, 7, 9, 11, 12, 13, 14, 15]
    s, d = to.partition(torch.tensor([3, 0, 1, 2, 0, 3], dtype=torch.uint8), 4, 6)      # non-square: 2 x 3 cells
    assert d.tolist() == [7, 2, 5, 18, 14, 23] and len(s) == 18 and sorted(s.tolist() + d.tolist()) == list(range(24))


def _grid(seed=0, B=2, C=8):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, 16, C, generator=g, dtype=torch.float64)


def test_r_zero_is_the_identity_and_unmerge_restores_kept_and_dst_rows():
    x = _grid()
    m = to.match(x, torch.tensor([0, 1, 2, 3], dtype=torch.uint8), 4, 4, 0)
    args = (m["src_tok"], m["dst_tok"], m["kept"], m["merged"], m["dst_idx"])
    assert m["merged"].shape == (2, 0) and m["kept"].tolist() == [list(range(12))] * 2
    y = to.merge(x, *args)
    assert y.shape == x.shape and torch.equal(y, torch.cat([x[:, m["src_tok"]], x[:, m["dst_tok"]]], 1))     # a permutation
    assert torch.equal(to.unmerge(y, *args), x)


def test_the_mean_includes_the_dst_and_merged_tokens_read_their_dst():
    C = 4
    x = torch.zeros(1, 16, C, dtype=torch.float64)
    src, dst = to.partition(torch.zeros(4, dtype=torch.uint8), 4, 4)           # dst tokens 0, 2, 8, 10
    for i, t in enumerate(dst.tolist()):
        x[0, t, i] = 1.0                                                        # dst rows: the unit vectors e_i
    x[0, 1] = torch.tensor([4.0, 0.0, 0.0, 0.0])                               # src slot 0 -> dst 0, score 1
    x[0, 3] = torch.tensor([0.0, 3.0, 0.25, 0.0])                              # src slot 1 -> dst 1, score 0.9965
    x[0, 4] = torch.tensor([2.0, 0.0, 0.0, 0.0])                               # src slot 2 -> dst 0, score 1 (tie with slot 0)
    x[0, 5] = torch.tensor([0.0, 0.0, 1.0, 1.0])                               # src slot 3: ties dst 2 and 3 -> the lower, 0.707
    m = to.match(x, torch.zeros(4, dtype=torch.uint8), 4, 4, 3)
    assert m["node_idx"][0, :4].tolist() == [0, 1, 0, 2]
    assert m["node_idx"][0, 4:].tolist() == [0] * 8                             # zero rows: all scores 0, the lowest dst
    assert not torch.isnan(m["node_max"]).any() and m["node_max"][0, 4:].abs().max() == 0
    assert m["merged"].tolist() == [[0, 1, 2]] and m["dst_idx"].tolist() == [[0, 1, 0]]
    assert m["kept"].tolist() == [[3, 4, 5, 6, 7, 8, 9, 10, 11]]
    args = (m["src_tok"], m["dst_tok"], m["kept"], m["merged"], m["dst_idx"])
    y = to.merge(x, *args)
    assert y.shape == (1, 13, C)
    assert torch.equal(y[0, 9], torch.tensor([7.0 / 3, 0, 0, 0], dtype=torch.float64))          # (e_0 + 4 e_0 + 2 e_0) / 3
    assert torch.equal(y[0, 10], torch.tensor([0, 2.0, 0.125, 0], dtype=torch.float64))         # (e_1 + [0, 3, .25, 0]) / 2
    assert torch.equal(y[0, 11], x[0, 8]) and torch.equal(y[0, 12], x[0, 10])                  # no members: unchanged
    assert to.member_counts(m["dst_idx"], 4).tolist() == [[3, 2, 1, 1]]
    u = to.unmerge(y, *args)
    assert torch.equal(u[0, 1], y[0, 9]) and torch.equal(u[0, 4], y[0, 9]) and torch.equal(u[0, 0], y[0, 9])
    assert torch.equal(u[0, 3], y[0, 10]) and torch.equal(u[0, 5], x[0, 5])


def test_ratio_075_merges_every_src_and_the_cut_prefers_the_lowest_src():
    assert to.num_merged(16, 0.75) == 12 and to.num_merged(16, 0.5) == 8 and to.num_merged(48, 0.3) == 14
    assert to.num_merged(4096, 0.5) == 2048 and to.num_merged(16, 0.0) == 0
    x = _grid(seed=3)
    m = to.match(x, torch.tensor([1, 1, 2, 0], dtype=torch.uint8), 4, 4, to.num_merged(16, 0.75))
    assert m["kept"].shape == (2, 0) and m["merged"].tolist() == [list(range(12))] * 2
    y = to.merge(x, m["src_tok"], m["dst_tok"], m["kept"], m["merged"], m["dst_idx"])
    assert y.shape == (2, 4, 8)
    cnt = to.member_counts(m["dst_idx"], 4)
    assert cnt.sum(1).tolist() == [16, 16]
    for b in range(2):          # every dst row is the mean of its group, and the groups partition the tokens
        for d in range(4):
            members = [int(m["dst_tok"][d])] + [int(m["src_tok"][s]) for s, dd in zip(m["merged"][b], m["dst_idx"][b]) if dd == d]
            assert torch.allclose(y[b, d], x[b, members].mean(0), atol=1e-14)
    kept, merged = to.select(torch.tensor([[0.5, 0.9, 0.5, -0.0, 0.0, 0.5]]), 3)      # ties at the cut: the lowest src slots
    assert merged.tolist() == [[0, 1, 2]] and kept.tolist() == [[3, 4, 5]]
    kept, merged = to.select(torch.tensor([[0.0, -0.0, -1.0, 0.0]]), 2)               # -0 and +0 are one value
    assert merged.tolist() == [[0, 1]]


@pytest.mark.parametrize("h,w", [(16, 16), (16, 24)])
def test_oracle_forward_with_tome_off_is_the_plain_oracle_and_with_tome_differs(h, w):
    """The with / without distance the GPU test asks for (> 10 x UNET_TOL = 0.2) is checked here first, at its shapes and
    weights (measured: 0.30 at 16x16, 0.25 at 16x24 with max_downsample 1; 0.31 / 0.26 with 2)."""
    from oracle.unet import unet_forward
    from sonicdiffusionbayeslab_amd.weights import UNetConfig, make_synthetic_state_dict
    from tests.util import oracle_cfg, rel_l2
    cfg = UNetConfig(sample_size=16)
    sd = to.tome_test_weights(make_synthetic_state_dict(cfg, seed=1234))
    g = torch.Generator().manual_seed(29)
    lat, pe = torch.randn(1, 4, h, w, generator=g), torch.randn(1, 77, 768, generator=g)
    with torch.no_grad():
        plain = unet_forward(sd, oracle_cfg(cfg), lat, 981.0, pe)
    off = to.unet_forward(sd, oracle_cfg(cfg), lat, 981.0, pe, to.TomeRun((h, w), 0.0, 1, []))
    assert torch.equal(off, plain)
    cells = (h // 2) * (w // 2)
    # five level-0 blocks: down 0.0, 0.1, up 3.0, 3.1, 3.2; a RANDOM dst choice, as the GPU test draws it (with the top-left token
    # of every cell the kept tokens are a regular sub-grid and the distance at 16x24 is 0.14 .. 0.15 at any gain)
    gc = torch.Generator().manual_seed(5)
    choices = [torch.randint(4, (cells,), generator=gc, dtype=torch.uint8) for _ in range(5)]
    run = to.TomeRun((h, w), 0.5, 1, choices)
    on = to.unet_forward(sd, oracle_cfg(cfg), lat, 981.0, pe, run)
    assert len(run.used) == 5 and all(m["merged"].shape == (1, h * w // 2) for m in run.used)
    again = to.unet_forward(sd, oracle_cfg(cfg), lat, 981.0, pe, to.TomeRun((h, w), 0.5, 1, choices, given=run.used))
    assert torch.equal(again, on)                                 # fed its own matchings back: the same forward
    d = rel_l2(on, plain)
    print(f"oracle with / without Token Merging at {h}x{w}, ratio 0.5:", d)
    assert d > 0.2, d


_ENVS, _PLAIN = {}, {}          # per UNet its weights, per (UNet, shape, batch, seed, timestep) the plain forward: computed once


@pytest.mark.parametrize("name,h,w,lb,ub,md,ratio,n_blocks,seed,t", to.UNET_CASES,
                         ids=[f"{c[0]}-{c[1]}x{c[2]}-b{c[3]}_{c[4]}-r{c[6]}" for c in to.UNET_CASES])
def test_oracle_with_without_distance_at_every_unet_case_of_the_gpu_tests(name, h, w, lb, ub, md, ratio, n_blocks, seed, t):
    """The same check at every (UNet, shape, ratio, batch) tests/test_tome_gpu.py runs beyond ratio 0.5 at 16x16 / 16x24, with
    the oracle alone (it matches on its own), at the GPU test's inputs (tome_oracle.unet_inputs) and against the floor the GPU
    test uses (tome_oracle.moved_floor: 0.2 from ratio 0.5 on, 0.1 below).  Measured: sd15 16x16 0.170 / 0.184 / 0.306 at ratios
    0.25 / 0.3 / 0.75, 16x24 0.157 / 0.186 / 0.327; sd2 16x16 at 0.3 0.394; two_level 32x32 at ratio 0.5 0.228 (batch 16/16) and
    0.235 (8/16), at 0.25 0.148 and 0.161."""
    from tests.util import rel_l2
    if name not in _ENVS:
        _ENVS[name] = to.unet_env(name)
    cfg, sd, ocfg, heads = _ENVS[name]
    lat, ctx, sample, choice = to.unet_inputs(cfg, h, w, lb, ub, md, seed)
    grids = to.merging_grids(cfg, h, w, md)
    assert len(grids) == n_blocks and sample.shape[0] == ub
    key = (name, h, w, lb, ub, seed, t)
    if key not in _PLAIN:
        _PLAIN[key] = to.unet_forward(sd, ocfg, sample, t, ctx, to.TomeRun((h, w), 0.0, md, []), heads_per_level=heads)
    run = to.TomeRun((h, w), ratio, md, choice)
    on = to.unet_forward(sd, ocfg, sample, t, ctx, run, heads_per_level=heads)
    assert [(m["src_tok"].numel() + m["dst_tok"].numel()) for m in run.used] == [a * b for a, b in grids]      # call order, all consumed
    assert sum(c.numel() for c in run.choices) == choice.numel()
    for m, (a, b) in zip(run.used, grids):
        assert m["merged"].shape == (ub, to.num_merged(a * b, ratio)) and m["kept"].shape == (ub, a * b - a * b // 4 - m["r"])
    d = rel_l2(on, _PLAIN[key])
    print(f"oracle with / without Token Merging, {name} {h}x{w} batch {lb}/{ub} ratio {ratio}: {d:.3f} (floor {to.moved_floor(ratio)})")
    assert d > to.moved_floor(ratio), d


def test_merging_grids_and_the_floor():
    from sonicdiffusionbayeslab_amd.weights import UNetConfig
    cfg = UNetConfig(sample_size=16)
    assert to.merging_grids(cfg, 16, 24, 1) == [(16, 24)] * 5
    assert to.merging_grids(cfg, 16, 24, 2) == [(16, 24)] * 2 + [(8, 12)] * 5 + [(16, 24)] * 3
    two = UNetConfig(sample_size=32, block_out_channels=(320, 640), attn_levels=(True, True))
    assert to.merging_grids(two, 32, 32, 1) == [(32, 32)] * 5                  # the mid block sits on level 1
    assert to.merging_grids(two, 32, 32, 2) == [(32, 32)] * 2 + [(16, 16)] * 6 + [(32, 32)] * 3
    assert to.moved_floor(0.25) == to.moved_floor(0.3) == 5 * to.UNET_TOL and to.moved_floor(0.5) == to.moved_floor(0.75) == 10 * to.UNET_TOL
    assert to.UNET_TOL == 2e-2


# ------------------------------------------------------------------------------------------------- registry, YAML, refusals
def test_registry_key_and_yaml_keys():
    import os
    from sonicdiffusionbayeslab_amd.config import load_config
    from sonicdiffusionbayeslab_amd.experiments.base_experiment import BaseMethod
    from sonicdiffusionbayeslab_amd.registry import methods_registry
    assert "tome" in methods_registry
    cfg = load_config(os.path.join(os.path.dirname(__file__), "..", "configs", "tome_config.yaml"))
    assert cfg.experiment.method == "tome" and list(cfg.experiment_params.tome_ratio) == [0.0, 0.25, 0.5, 0.75]
    from sonicdiffusionbayeslab_amd.config import _wrap
    assert BaseMethod.parse_tome(_wrap({"model_name": "x"})) is None
    got = BaseMethod.parse_tome(_wrap({"tome_ratio": 0.5, "tome_max_downsample": 2, "tome_use_rand": False, "tome_seed": 7}))
    assert got == dict(ratio=0.5, max_downsample=2, use_rand=False, seed=7)
    assert BaseMethod.parse_tome(_wrap({"tome_ratio": 0.25})) == dict(ratio=0.25, max_downsample=1, use_rand=True, seed=0)
    with pytest.raises(ValueError, match="tome_seed"):
        BaseMethod.parse_tome(_wrap({"tome_seed": 3}))


def test_every_refusal_by_name_before_any_gpu_work():
    from sonicdiffusionbayeslab_amd.models import StableDiffusionModel as M
    m = M()
    for bad in (-0.1, 0.76, 1.0, "0.5", True):
        with pytest.raises(ValueError, match="ratio"):
            m.apply_tome(ratio=bad)
    with pytest.raises(NotImplementedError, match="sx"):
        m.apply_tome(sx=4)
    with pytest.raises(NotImplementedError, match="sy"):
        m.apply_tome(sy=1)
    for bad in (0, 4, 8):
        with pytest.raises(NotImplementedError, match="max_downsample"):
            m.apply_tome(max_downsample=bad)
    with pytest.raises(NotImplementedError, match="merge_crossattn"):
        m.apply_tome(merge_crossattn=True)
    with pytest.raises(NotImplementedError, match="merge_mlp"):
        m.apply_tome(merge_mlp=True)
    with pytest.raises(NotImplementedError, match="merge_attn"):
        m.apply_tome(merge_attn=False)
    with pytest.raises(ValueError, match="rand_every"):
        m.apply_tome(rand_every="block")
    with pytest.raises(NotImplementedError, match="fp8"):
        M(weight_dtype="fp8").apply_tome(ratio=0.5)
    assert m._tome is None                                         # nothing above took effect
    assert m.apply_tome(ratio=0.75, max_downsample=2, seed=5, rand_every="call") is m
    assert m._tome == dict(ratio=0.75, max_downsample=2, use_rand=True, seed=5, rand_every="call")
    m.apply_tome(ratio=0)                                          # ratio 0 is remove_tome()
    assert m._tome is None
    m.apply_tome()
    assert m._tome["ratio"] == 0.5 and m.remove_tome() is m and m._tome is None
    assert M(weight_dtype="fp8").apply_tome(ratio=0.0)._tome is None          # off is never refused


def test_choice_arrays_depend_on_the_seed_alone(monkeypatch):
    from sonicdiffusionbayeslab_amd.models import StableDiffusionModel as M
    draws = {}
    for world, rank in ((1, 0), (2, 0), (2, 1), (8, 5)):
        monkeypatch.setenv("WORLD_SIZE", str(world))
        monkeypatch.setenv("RANK", str(rank))
        g = torch.Generator().manual_seed(11)
        draws[(world, rank)] = [M.draw_tome_choice(g, 5 * 64) for _ in range(3)]       # three forwards of five blocks
    first = draws[(1, 0)]
    assert all(c.dtype == torch.uint8 and c.shape == (320,) and int(c.max()) <= 3 for c in first)
    assert not torch.equal(first[0], first[1])                     # a fresh draw per forward
    for d in draws.values():
        assert all(torch.equal(a, b) for a, b in zip(d, first))
    other = M.draw_tome_choice(torch.Generator().manual_seed(12), 320)
    assert not torch.equal(other, first[0])


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
        assert lib.sd_unet_set_tome(h, 0.5, 1) == 0 and lib.sd_unet_set_tome(h, 0.75, 2) == 0 and lib.sd_unet_set_tome(h, 0.0, 0) == 0
        for ratio, md in ((0.8, 1), (-0.5, 1), (0.5, 0), (0.5, 4)):
            assert lib.sd_unet_set_tome(h, ratio, md) != 0
            assert b"set_tome" in lib.sd_last_error()
    finally:
        lib.sd_unet_destroy(h)
    fp8 = _c_config(UNetConfig(sample_size=16), "fp8")
    _lib.check(lib.sd_unet_create(C.byref(fp8), C.byref(h)), "sd_unet_create")
    try:
        assert lib.sd_unet_set_tome(h, 0.5, 1) != 0 and b"fp8" in lib.sd_last_error()
        assert lib.sd_unet_set_tome(h, 0.0, 0) == 0
    finally:
        lib.sd_unet_destroy(h)
    # the kernels' entry points check their shapes on the host, before any launch
    assert lib.sd_op_tome_match(None, None, None, 1, 7, 8, 320, None, None, None) != 0 and b"even sides" in lib.sd_last_error()
    assert lib.sd_op_tome_select(None, 1, 1, 1, 20000, 5, 1, 1, 1) != 0 and b"12288" in lib.sd_last_error()
    assert lib.sd_op_tome_merge(None, 1, 1, 1, 1, 1, 1, 300, 1, 8, 8, 300, 4) != 0 and b"multiple of 64" in lib.sd_last_error()
