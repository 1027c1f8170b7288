"""HyperTile without a GPU: the tiling rule worked by hand, the gather / scatter index maps against reshape / permute, the oracle
(tests/hypertile_oracle.py) with the setting off and its tiled-against-plain distance at every UNet case of the GPU tests, every
refusal by name, the registry key and YAML keys, the exported symbols and the shape rule ``sd_hypertile_check``."""
import os

import pytest
import torch

from sonicdiffusionbayeslab_amd import _lib
from tests import hypertile_oracle as ho

NEW_SYMBOLS = ["sd_unet_set_hypertile", "sd_unet_hypertile_block_count_hw", "sd_unet_hypertile_block_info_hw", "sd_hypertile_check",
               "sd_op_hypertile_gather", "sd_op_hypertile_scatter"]


# ----------------------------------------------------------------------------------------------------------- tiling rule
def test_tiling_rule_by_hand():
    # T = 32 tokens (tile_size 256 px).  128: 32 divides it, 4 tiles; 96: 3 tiles of 32; 64: 2 tiles; 40: no divisor in [32, 40),
    # the smallest divisor >= 32 is 40 itself, one tile
    assert [ho.tile_side(r, 32) for r in (128, 96, 64, 40)] == [32, 32, 32, 40]
    assert ho.tiling(128, 128, 32) == (4, 4, 32, 32) and ho.tiling(64, 96, 32) == (2, 3, 32, 32)
    assert ho.tiling(40, 40, 32) == (1, 1, 40, 40) and ho.tiling(64, 40, 32) == (2, 1, 32, 40)
    assert ho.tiling(16, 24, 8) == (2, 3, 8, 8)
    # a side below T is one tile; a T that divides nothing takes the next divisor up
    assert ho.tile_side(16, 32) == 16 and ho.tile_side(48, 20) == 24 and ho.tile_side(36, 10) == 12 and ho.tile_side(34, 3) == 17
    # the rule's defining properties on every side up to 128
    for T in (8, 12, 16, 32, 48):
        for r in range(1, 129):
            th = ho.tile_side(r, T)
            assert r % th == 0 and th >= min(T, r) and not any(r % d == 0 for d in range(min(T, r), th))


def test_which_blocks_tile_at_the_issue_examples():
    from sonicdiffusionbayeslab_amd.weights import UNetConfig
    cfg = UNetConfig(sample_size=64)
    # 1024 px, tile_size 256, max_depth 1: the 128x128 level runs 16 tiles of 1024 tokens, the 64x64 level 4 tiles of 1024
    g = ho.tiled_grids(cfg, 128, 128, 32, 1)
    assert g == [(128, 128, 4, 4)] * 2 + [(64, 64, 2, 2)] * 5 + [(128, 128, 4, 4)] * 3
    assert all((rh // nh) * (rw // nw) == 1024 for rh, rw, nh, nw in g)
    # 512x768 px, max_depth 0: the 64x96 level runs 2x3 tiles of 1024 tokens, nothing deeper
    assert ho.tiled_grids(cfg, 64, 96, 32, 0) == [(64, 96, 2, 3)] * 5
    # 320 px: one tile, nothing is tiled -- and at max_depth 3 neither (20, 10, 5 tokens)
    assert ho.tiled_grids(cfg, 40, 40, 32, 0) == [] and ho.tiled_grids(cfg, 40, 40, 32, 3) == []
    # off
    assert ho.tiled_grids(cfg, 128, 128, 0, 3) == []
    # the cases of the GPU file
    for name, h, w, lb, ub, seed, t, T, md, n in ho.UNET_CASES + [ho.SD2_CASE]:
        assert len(ho.tiled_grids(ho.env(name)[0], h, w, T, md)) == n


@pytest.mark.parametrize("rh,rw,nh,nw", [(16, 24, 2, 3), (8, 8, 2, 2), (6, 10, 3, 5), (4, 4, 1, 1), (4, 6, 4, 1), (128, 128, 4, 4)])
def test_gather_and_scatter_index_maps_against_reshape_permute(rh, rw, nh, nw):
    th, tw = rh // nh, rw // nw
    g, s = ho.gather_index(rh, rw, nh, nw), ho.scatter_index(rh, rw, nh, nw)
    ids = torch.arange(rh * rw)
    want = ids.reshape(nh, th, nw, tw).permute(0, 2, 1, 3).reshape(-1)
    assert torch.equal(g, want)
    assert torch.equal(g.sort().values, ids) and torch.equal(g[s], ids) and torch.equal(s[g], ids)
    if nh * nw == 1:
        assert torch.equal(g, ids)
    x = torch.randn(3, rh * rw, 5, generator=torch.Generator().manual_seed(rh * 131 + rw))
    tiles = ho.to_tiles(x, rh, rw, nh, nw)
    assert tiles.shape == (3 * nh * nw, th * tw, 5)
    assert torch.equal(tiles.reshape(3, rh * rw, 5), x[:, g]) and torch.equal(ho.from_tiles(tiles, rh, rw, nh, nw), x)
    # tile (i, j), row (y, x) by the definition
    i, j, y, xx = nh - 1, nw // 2, th - 1, tw // 2
    assert torch.equal(tiles[1 * nh * nw + i * nw + j, y * tw + xx], x[1, (i * th + y) * rw + j * tw + xx])


# ------------------------------------------------------------------------------------------------------------ the oracle
def test_oracle_with_the_setting_off_is_the_plain_oracle():
    from oracle.unet import unet_forward
    name, h, w, lb, ub, seed, t, T, md, n = ho.UNET_CASES[0]
    cfg, sd, ocfg, heads = ho.env(name)
    lat, ctx, sample = ho.unet_inputs(cfg, h, w, lb, ub, seed)
    with torch.no_grad():
        plain = unet_forward(sd, ocfg, sample, t, ctx)
    assert torch.equal(ho.reference(ho.UNET_CASES[0])["plain"], plain)
    # a setting that tiles nothing (one tile per level) is the plain oracle too
    run = ho.TileRun((h, w), 16, 3)
    assert torch.equal(ho.unet_forward(sd, ocfg, sample, t, ctx, run), plain) and run.used == []


@pytest.mark.parametrize("case", ho.UNET_CASES + [ho.SD2_CASE], ids=lambda c: f"{c[0]}-{c[1]}x{c[2]}-b{c[3]}_{c[4]}-T{c[7]}-d{c[8]}")
def test_oracle_tiled_against_plain_distance_at_every_unet_case_of_the_gpu_tests(case):
    """With the oracle alone, at the GPU test's inputs and against the floor the GPU test uses, 5 x UNET_TOL = 0.10.  Measured:
    sd15 16x16 0.394, 16x24 0.403, 32x32 (T = 8, depth 2) 0.415; two_level 32x32 T = 16 0.219, T = 8 depth 1 0.533.  A forward
    that ignored the setting would miss UNET_TOL by at least a factor of ten on every one of them."""
    from tests.util import rel_l2
    name, h, w, lb, ub, seed, t, T, md, n = case
    ref = ho.reference(case)
    assert ref["used"] == ho.tiled_grids(ho.env(name)[0], h, w, T, md) and len(ref["used"]) == n
    d = rel_l2(ref["tiled"], ref["plain"])
    print(f"oracle tiled / plain, {name} {h}x{w} batch {lb}/{ub} T {T} max_depth {md}: {d:.3f} (floor {ho.FLOOR})")
    assert ho.FLOOR == 5 * 2e-2 and d > ho.FLOOR, d


# ------------------------------------------------------------------------------------------------- registry, YAML, refusals
def test_registry_key_and_yaml_keys():
    from sonicdiffusionbayeslab_amd.config import _wrap, load_config
    from sonicdiffusionbayeslab_amd.experiments.base_experiment import BaseMethod
    from sonicdiffusionbayeslab_amd.registry import methods_registry
    assert "hypertile" in methods_registry
    cfg = load_config(os.path.join(os.path.dirname(__file__), "..", "configs", "hypertile_config.yaml"))
    assert cfg.experiment.method == "hypertile" and list(cfg.experiment_params.hypertile_tile_size) == [None, 256]
    assert cfg.scheduler.scheduler_name == "ddim_scheduler" and cfg.experiment_params.height == cfg.experiment_params.width == 1024
    assert BaseMethod.parse_hypertile(_wrap({"model_name": "x"})) is None
    assert BaseMethod.parse_hypertile(_wrap({"hypertile": {"tile_size": 256, "max_depth": 1}})) == dict(tile_size=256, max_depth=1)
    assert BaseMethod.parse_hypertile(_wrap({"hypertile": {"tile_size": 128}})) == dict(tile_size=128, max_depth=0)
    with pytest.raises(ValueError, match="tile_size"):
        BaseMethod.parse_hypertile(_wrap({"hypertile": {"max_depth": 1}}))
    with pytest.raises(ValueError, match="swap_size"):
        BaseMethod.parse_hypertile(_wrap({"hypertile": {"tile_size": 256, "swap_size": 2}}))
    with pytest.raises(ValueError, match="mapping"):
        BaseMethod.parse_hypertile(_wrap({"hypertile": 256}))
    with pytest.raises(ValueError, match="tile_size"):
        BaseMethod.parse_hypertile(_wrap({"hypertile": {"tile_size": 100}}))
    with pytest.raises(NotImplementedError, match="fp8"):
        BaseMethod.parse_hypertile(_wrap({"hypertile": {"tile_size": 256}}), "fp8")


def test_every_refusal_by_name_before_any_gpu_work():
    from sonicdiffusionbayeslab_amd.models import StableDiffusionModel as M
    m = M()
    for bad in (100, 260, 56, 0, 8, -256, 256.0, "256", True, None):      # not a multiple of 8, below 64, not an integer
        with pytest.raises(ValueError, match="tile_size"):
            m.enable_hypertile(tile_size=bad)
    for bad in (-1, 4, 1.0, "1", True, None):
        with pytest.raises(ValueError, match="max_depth"):
            m.enable_hypertile(max_depth=bad)
    for bad in (0, 2, 3, None):
        with pytest.raises(NotImplementedError, match="swap_size"):
            m.enable_hypertile(swap_size=bad)
    with pytest.raises(NotImplementedError, match="fp8"):
        M(weight_dtype="fp8").enable_hypertile()
    assert m._hypertile is None                                    # nothing above took effect
    # Token Merging and HyperTile together, either order
    m.apply_tome(ratio=0.5)
    with pytest.raises(NotImplementedError, match="Token Merging"):
        m.enable_hypertile()
    m.remove_tome()
    assert m.enable_hypertile() is m and m._hypertile == (32, 0)
    with pytest.raises(NotImplementedError, match="HyperTile"):
        m.apply_tome(ratio=0.5)
    assert m._tome is None
    m.apply_tome(ratio=0)                                          # switching Token Merging OFF is never refused
    assert m.enable_hypertile(tile_size=128, max_depth=3)._hypertile == (16, 3)
    assert m.enable_hypertile(tile_size=64)._hypertile == (8, 0)
    assert m.disable_hypertile() is m and m._hypertile is None
    assert M(weight_dtype="fp8").disable_hypertile()._hypertile is None       # off is never refused
    # the UNet wrapper's own argument check (tokens, not pixels)
    from sonicdiffusionbayeslab_amd.unet import HipUNet2DConditionModel as U
    assert U.check_hypertile_args(0, 0) is None and U.check_hypertile_args(0, 99) is None and U.check_hypertile_args(32, 1) == (32, 1)
    for bad in (7, 1, -8, 257, 8.0, True):
        with pytest.raises(ValueError, match="tile_tokens"):
            U.check_hypertile_args(bad, 0)
    with pytest.raises(ValueError, match="max_depth"):
        U.check_hypertile_args(8, 4)
    with pytest.raises(NotImplementedError, match="fp8"):
        U.check_hypertile_args(8, 0, "fp8")


def test_the_experiment_refuses_bad_sweeps_by_name():
    from sonicdiffusionbayeslab_amd.config import _wrap
    from sonicdiffusionbayeslab_amd.experiments.hypertile import HyperTileMethod
    m = HyperTileMethod.__new__(HyperTileMethod)
    m.config = _wrap({"model": {}, "experiment_params": {"hypertile_tile_size": [None, 256, 128], "hypertile_max_depth": 1,
                                                        "height": 1024, "width": 768, "num_inference_steps": [50]}})
    m.setup_exp_params()
    assert m.hypertile_tile_size == [None, 256, 128] and m.hypertile_max_depth == 1 and m.size_kwargs == dict(height=1024, width=768)
    for bad, match in (({"hypertile_tile_size": 256}, "list"), ({"hypertile_tile_size": [100]}, "tile_size"),
                       ({"hypertile_tile_size": [256], "hypertile_max_depth": 4}, "max_depth")):
        m.config = _wrap({"model": {}, "experiment_params": {"num_inference_steps": [50], **bad}})
        with pytest.raises(ValueError, match=match):
            m.setup_exp_params()
    m.config = _wrap({"model": {"weight_dtype": "fp8"}, "experiment_params": {"num_inference_steps": [50], "hypertile_tile_size": [256]}})
    with pytest.raises(NotImplementedError, match="fp8"):
        m.setup_exp_params()


# ------------------------------------------------------------------------------------------------------------- the C ABI
def test_symbols_are_exported_and_the_abi_version_stays():
    lib = _lib.load()
    for s in NEW_SYMBOLS:
        assert s in _lib._SIGS and hasattr(lib, s), s
    assert lib.sd_abi_version() == 3


def test_sd_hypertile_check_refuses_bad_shapes_without_a_gpu():
    lib = _lib.load()
    ok = [(2, 16, 24, 320, 2, 3, 320), (3, 8, 8, 1280, 2, 2, 1280), (1, 6, 10, 64, 3, 5, 64), (1, 128, 128, 320, 4, 4, 328),
          (1, 256, 256, 8, 1, 1, 8), (65535, 1, 1, 16384, 1, 1, 1 << 30), (2, 128, 128, 64, 4, 4, 65552)]
    for a in ok:
        assert lib.sd_hypertile_check(*a) == 0, a
    bad = [((0, 16, 24, 320, 2, 3, 320), "B="), ((65536, 16, 24, 320, 2, 3, 320), "B="),
           ((1, 0, 24, 320, 1, 3, 320), "tokens"), ((1, 16, 257, 320, 2, 1, 320), "tokens"),
           ((1, 16, 24, 320, 3, 3, 320), "tiles"), ((1, 16, 24, 320, 2, 5, 320), "tiles"), ((1, 16, 24, 320, 0, 3, 320), "tiles"),
           ((1, 16, 24, 0, 2, 3, 320), "C="), ((1, 16, 24, 324, 2, 3, 328), "C="), ((1, 16, 24, 16392, 2, 3, 16392), "C="),
           ((1, 16, 24, 320, 2, 3, 312), "pitch"), ((1, 16, 24, 320, 2, 3, 324), "pitch"), ((1, 16, 24, 320, 2, 3, -320), "pitch"),
           ((1, 16, 24, 320, 2, 3, (1 << 30) + 8), "pitch")]
    for a, what in bad:
        assert lib.sd_hypertile_check(*a) == -1, a
        msg = lib.sd_last_error().decode()
        assert msg.startswith("sd_hypertile_check:") and what in msg, (a, msg)


# ------------------------------------------------------------------------------- the sharded harness at a non-default size
class _StubOut:
    def __init__(self, images):
        self.images = images


class _StubPipeline:
    """A per-image function of (prompt, the Gaussian a call draws, the setting) at the call's size; the UNet's own size is 64 px."""
    weights_source = "stub"
    num_timesteps = 3

    def __init__(self):
        from sonicdiffusionbayeslab_amd.schedulers import SchedulerConfig
        from sonicdiffusionbayeslab_amd.weights import UNetConfig
        self.unet_config = UNetConfig(sample_size=8)
        self.scheduler = type("S", (), {})()
        self.scheduler.config = SchedulerConfig()
        self.tile, self.seen = None, []

    def to(self, device):
        return self

    def enable_hypertile(self, tile_size=256, max_depth=0):
        self.tile = (tile_size, max_depth)

    def disable_hypertile(self):
        self.tile = None

    def __call__(self, prompts, num_inference_steps=3, guidance_scale=7.5, generator=None, output_type="latent", height=None,
                 width=None, **kw):
        from sonicdiffusionbayeslab_amd import dist as sdist
        n = len(prompts)
        noise = sdist.randn((n, 4, height // 8, width // 8), generator)
        key = torch.tensor([float(sum(map(ord, p)) % 97) for p in prompts]).view(n, 1, 1, 1)
        self.seen.append((n, self.tile))
        return _StubOut(noise + key + (0.0 if self.tile is None else 1000.0)), 0.25, []


def _harness_run(tmp):
    """``methods_registry["hypertile"]`` over a stub pipeline: 3 prompts in batches of 2 at 128x192 px, off and then 64 px
    tiles; returns the latents every ``validate`` call received and the (shard size, setting) of every pipeline call."""
    import json
    from sonicdiffusionbayeslab_amd.config import _wrap
    from sonicdiffusionbayeslab_amd.experiments.hypertile import HyperTileMethod
    got = []

    class M(HyperTileMethod):
        def setup_model(self):
            self.model = _StubPipeline()

        def setup_scheduler(self, **kw):
            pass

        def validate(self, name, additional_values=None, n_images=0, images=None, **kw):
            got.append((additional_values["HyperTile"], torch.stack(images)))
    from PIL import Image
    os.makedirs(os.path.join(tmp, "img"), exist_ok=True)
    for i in range(3):
        Image.new("RGB", (16, 16), (40 * i, 0, 0)).save(os.path.join(tmp, "img", f"im{i}.png"))
    with open(os.path.join(tmp, "prompts.json"), "w") as f:
        json.dump({f"im{i}.png": f"prompt number {i}" for i in range(3)}, f)
    conf = {"experiment_name": "stub", "experiment": {"method": "hypertile", "seed": 29}, "model": {},
            "dataset": {"img_dataset": os.path.join(tmp, "img"), "prompts": os.path.join(tmp, "prompts.json"), "image_size": 64},
            "inference": {"batch_size": 2, "output_type": "latent"},
            "experiment_params": {"hypertile_tile_size": [None, 64], "height": 128, "width": 192, "num_inference_steps": [3]}}
    m = M(_wrap(conf))
    m.test_dataset.image_files = sorted(m.test_dataset.image_files)
    m.run_experiment()
    return got, list(m.model.seen)


def _free_port():
    import socket
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close(); return p


def _harness_worker(rank, world, port, tmp, q):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank), SD_DIST_BACKEND="gloo")
    got, seen = _harness_run(os.path.join(tmp, f"rank{rank}"))
    q.put((rank, [(label, t.numpy()) for label, t in got], seen))
    dist.barrier()
    dist.destroy_process_group()


def test_sharded_harness_with_more_ranks_than_prompts_at_a_non_default_size(tmp_path):
    """Three ranks over gloo, batches of 2 and 1 prompts at 128x192 px on a UNet whose own size is 64 px: in every batch at least
    one rank has no prompt and enters the all-gather with an empty result, which must have the CALL's row size ([0, 4, 16, 24]),
    not the UNet's ([0, 4, 8, 8]) -- ranks that disagree on the element count leave the collective undefined.  Every rank ends
    with the single-process result, every image is computed once, under both settings of the sweep."""
    import torch.multiprocessing as mp
    tmp = str(tmp_path)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        os.environ.pop(k, None)
    want, seen = _harness_run(os.path.join(tmp, "single"))
    assert [label for label, _ in want] == ["off", "64 px, max_depth 0"] and all(t.shape == (3, 4, 16, 24) for _, t in want)
    assert seen == [(2, None), (1, None), (2, (64, 0)), (1, (64, 0))]
    assert float((want[1][1] - want[0][1]).min()) > 900.0                 # the second sweep point ran with the setting on
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    ps = [ctx.Process(target=_harness_worker, args=(r, 3, port, tmp, q), daemon=True) for r in range(3)]
    [p.start() for p in ps]
    try:
        outs = {r: (g, s) for r, g, s in (q.get(timeout=120) for _ in range(3))}
    finally:          # (ranks that disagree on the collective's size hang in it: never leave them behind)
        [p.join(30) for p in ps]
        [p.kill() for p in ps if p.is_alive()]
    assert all(p.exitcode == 0 for p in ps)
    for r in range(3):
        for (label, t), (wl, wt) in zip(outs[r][0], want):
            assert label == wl and torch.equal(torch.from_numpy(t), wt), (r, label)
    calls = [c for r in range(3) for c in outs[r][1]]
    assert sum(n for n, tile in calls if tile is None) == 3 and sum(n for n, tile in calls if tile is not None) == 3
    assert any(len(outs[r][1]) < 4 for r in range(3))                     # some rank sat a batch out
