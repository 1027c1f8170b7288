"""FID without a GPU: registry and constructor errors, the exported symbols, the Frechet distance against an independent
scipy evaluation, the oracle's resize on hand-computed cases, the layer table, and the metric's state logic."""
import os

import numpy as np
import pytest
import torch

from sonicdiffusionbayeslab_amd import _lib
from sonicdiffusionbayeslab_amd.registry import metrics_registry
from tests import fid_util, inception_oracle

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fid_golden.npz")


@pytest.fixture(scope="module")
def weights_file(tmp_path_factory):
    p = tmp_path_factory.mktemp("fid") / "inception.pth"
    torch.save(fid_util.random_state_dict(0), str(p))
    return str(p)


def test_fid_is_registered():
    assert "fid" in metrics_registry
    from sonicdiffusionbayeslab_amd.metrics import FID
    assert metrics_registry["fid"] is FID


def test_constructor_errors(weights_file, tmp_path):
    FID = metrics_registry["fid"]
    for bad in (63, 1024, "2048", None, True):
        with pytest.raises(ValueError, match="64, 192, 768, 2048"):
            FID(feature=bad, weights=weights_file)
    with pytest.raises(FileNotFoundError, match="local checkpoint file"):
        FID(feature=64)
    with pytest.raises(FileNotFoundError, match="local checkpoint file"):
        FID(feature=64, weights=str(tmp_path / "absent.pth"))
    with pytest.raises(FileNotFoundError):
        FID(feature=64, weights=str(tmp_path))                 # a directory is not a checkpoint file
    m = FID(feature=192, input_img_size=(3, 299, 299), weights=weights_file)   # input_img_size: accepted, ignored
    assert m.feature == 192 and m.feature_fn is None            # the network is not built before the first update


def test_new_symbols_are_exported_and_declared():
    lib = _lib.load()
    names = ["sd_inception_create", "sd_inception_destroy", "sd_inception_num_convs", "sd_inception_conv_info",
             "sd_inception_load_conv", "sd_inception_finalize", "sd_inception_workspace_bytes", "sd_inception_features",
             "sd_fid_accumulate", "sd_op_inception_conv", "sd_op_maxpool3x3", "sd_op_avgpool3x3", "sd_op_global_mean",
             "sd_op_inception_resize"]
    for n in names:
        assert hasattr(lib, n), n
        assert n in _lib._SIGS and n in _lib.declared_symbols(), n
    assert lib.sd_abi_version() == 3


def test_library_layer_table_is_the_fid_inception():
    from sonicdiffusionbayeslab_amd.fid import conv_table
    want = [(n, (o, i, kh, kw)) for n, o, i, kh, kw in fid_util.layer_table()]
    assert len(want) == 94
    assert conv_table() == want


def test_state_dict_errors_name_the_key():
    from sonicdiffusionbayeslab_amd.fid import fold_state_dict
    sd = fid_util.random_state_dict(0)
    folded = fold_state_dict(sd)
    assert len(folded) == 94 and not any(k.startswith("fc") for k in folded)
    w, b = folded["Mixed_6c.branch7x7dbl_3"]
    assert tuple(w.shape) == (160, 160, 1, 7) and tuple(b.shape) == (160,) and w.dtype == torch.float32
    # the fold: scale = gamma / sqrt(var + 1e-3)
    p = "Conv2d_3b_1x1"
    scale = sd[p + ".bn.weight"].double() / torch.sqrt(sd[p + ".bn.running_var"].double() + 1e-3)
    assert torch.allclose(folded[p][0].double(), sd[p + ".conv.weight"].double() * scale.view(-1, 1, 1, 1), rtol=1e-6, atol=0)
    assert torch.allclose(folded[p][1].double(), sd[p + ".bn.bias"].double() - sd[p + ".bn.running_mean"].double() * scale,
                          rtol=1e-6, atol=1e-7)
    miss = dict(sd)
    del miss["Mixed_7a.branch7x7x3_2.bn.running_var"]
    with pytest.raises(KeyError, match="Mixed_7a.branch7x7x3_2.bn.running_var"):
        fold_state_dict(miss)
    bad = dict(sd)
    bad["Mixed_5c.branch5x5_2.conv.weight"] = torch.zeros(64, 48, 3, 3)
    with pytest.raises(ValueError, match="Mixed_5c.branch5x5_2.conv.weight"):
        fold_state_dict(bad)
    bad = dict(sd)
    bad["Mixed_6a.branch3x3.bn.bias"] = torch.zeros(383)
    with pytest.raises(ValueError, match="Mixed_6a.branch3x3.bn.bias"):
        fold_state_dict(bad)


def test_load_state_dict_formats(weights_file, tmp_path):
    from safetensors.torch import save_file

    from sonicdiffusionbayeslab_amd.fid import load_state_dict
    sd = load_state_dict(weights_file)
    assert "Mixed_7c.branch_pool.conv.weight" in sd
    small = {"Conv2d_1a_3x3.conv.weight": torch.ones(32, 3, 3, 3)}
    save_file(small, str(tmp_path / "w.safetensors"))
    assert torch.equal(load_state_dict(str(tmp_path / "w.safetensors"))["Conv2d_1a_3x3.conv.weight"], small["Conv2d_1a_3x3.conv.weight"])
    with pytest.raises(FileNotFoundError):
        load_state_dict(str(tmp_path / "nothing.pth"))


# ---- Frechet distance ---------------------------------------------------------------------------------------------------

def _relu_features(n, d, seed, shift=0.0):
    g = torch.Generator().manual_seed(seed)
    mix = torch.randn(d, d, generator=g, dtype=torch.float64) / d ** 0.5
    return torch.relu(torch.randn(n, d, generator=g, dtype=torch.float64) @ mix + 0.3 + shift)


def _stats(f):
    return f.mean(0), torch.cov(f.t())


def _sqrtm_fid(mu1, s1, mu2, s2):
    from scipy import linalg
    covmean = linalg.sqrtm(s1.numpy() @ s2.numpy())
    return float(((mu1 - mu2) ** 2).sum() + s1.trace() + s2.trace() - 2.0 * np.trace(covmean).real)


@pytest.mark.parametrize("d,n,gate", [(64, 96, 1e-10), (192, 48, 1e-6), (64, 32, 1e-6)])
def test_frechet_distance_against_sqrtm(d, n, gate):
    from sonicdiffusionbayeslab_amd.fid import frechet_distance
    a, b = _stats(_relu_features(n, d, 1)), _stats(_relu_features(n, d, 2, shift=0.2))
    got = float(frechet_distance(*a, *b))
    want = _sqrtm_fid(*a, *b)
    print(f"[fid] D={d} N={n}: eig {got:.12g} sqrtm {want:.12g} rel {abs(got - want) / abs(want):.3e}")
    assert abs(got - want) <= gate * abs(want)
    assert float(frechet_distance(*a, *a)) <= 1e-9 * got


def test_frechet_distance_at_2048():
    from sonicdiffusionbayeslab_amd.fid import frechet_distance
    a, b = _stats(_relu_features(32, 2048, 3)), _stats(_relu_features(32, 2048, 4, shift=0.2))
    got = frechet_distance(*a, *b)
    assert got.dtype == torch.float64 and not torch.is_complex(got)
    assert torch.isfinite(got)


# ---- oracle -------------------------------------------------------------------------------------------------------------

def test_oracle_resize_hand_cases():
    r = inception_oracle.tf1_resize
    # 2x2 -> 3x3: scale 2/3, src = 0, 2/3, 4/3 -> lo = 0, 0, 1, hi = 1, 1, 1, d = 0, 2/3, 1/3 (hi clamps at the edge)
    x = torch.tensor([[[[10.0, 40.0], [70.0, 130.0]]]]).repeat(1, 3, 1, 1)
    d = np.float32(1.0) * np.float32(np.float32(2.0) / np.float32(3.0))
    d1 = np.float32(2.0) * np.float32(np.float32(2.0) / np.float32(3.0)) - np.float32(1.0)
    def lerp(a, b, t):
        return np.float32(np.float32(a) + np.float32(np.float32(b) - np.float32(a)) * np.float32(t))
    top = [10.0, lerp(10, 40, d), lerp(40, 40, d1)]
    bot = [70.0, lerp(70, 130, d), lerp(130, 130, d1)]
    want = np.array([top, [lerp(t, b, d) for t, b in zip(top, bot)], [lerp(b, b, d1) for b in bot]], dtype=np.float32)
    got = r(x, side=3)
    assert got.shape == (1, 3, 3, 3)
    assert np.array_equal(got[0, 0].numpy(), want), (got[0, 0], want)
    assert abs(float(got[0, 0, 1, 1]) - (10 + 30 * 2 / 3 + (70 + 60 * 2 / 3 - 10 - 30 * 2 / 3) * 2 / 3)) < 1e-4
    # identity at 299
    img = fid_util.seeded_images(1, 299, 299, 3)
    assert torch.equal(r(img), img.float())
    # a 1x1 image: every output pixel is that value
    one = torch.tensor([7, 130, 255], dtype=torch.uint8).view(1, 3, 1, 1)
    out = r(one)
    assert out.shape == (1, 3, 299, 299) and torch.equal(out, one.float().expand(1, 3, 299, 299))
    assert torch.equal(inception_oracle.preprocess(one)[0, :, 0, 0], (torch.tensor([7.0, 130.0, 255.0]) - 128) / 128)


@pytest.fixture(scope="module")
def oracle_run():
    o = inception_oracle.Oracle(fid_util.random_state_dict(0))
    real, _ = fid_util.metric_images()
    return o, o.forward(real[:2])


def test_oracle_shapes_and_layer_table(oracle_run):
    o, taps = oracle_run
    assert {t: tuple(v.shape) for t, v in taps.items()} == {64: (2, 64), 192: (2, 192), 768: (2, 768), 2048: (2, 2048)}
    s = o.shapes
    sides = {"Conv2d_1a_3x3": 149, "Conv2d_2a_3x3": 147, "Conv2d_2b_3x3": 147, "Conv2d_3b_1x1": 73, "Conv2d_4a_3x3": 71,
             "Mixed_5b": 35, "Mixed_5c": 35, "Mixed_5d": 35, "Mixed_6a": 17, "Mixed_6e": 17, "Mixed_7a": 8, "Mixed_7c": 8}
    for name, side in sides.items():
        assert s[name][2:] == (side, side), (name, s[name])
    widths = {"Mixed_5b": 256, "Mixed_5c": 288, "Mixed_5d": 288, "Mixed_6a": 768, "Mixed_6b": 768, "Mixed_6c": 768,
              "Mixed_6d": 768, "Mixed_6e": 768, "Mixed_7a": 1280, "Mixed_7b": 2048, "Mixed_7c": 2048}
    for name, wd in widths.items():
        assert s[name][1] == wd, (name, s[name])
    # every conv of the table ran once, with the table's output width
    for name, cout, _, _, _ in fid_util.layer_table():
        assert s[name][1] == cout, name


def test_random_weights_keep_the_network_alive(oracle_run):
    _, taps = oracle_run
    f = taps[2048]
    assert torch.isfinite(f).all()
    assert float((f != 0).float().mean()) > 0.25
    assert float(f.abs().max()) < 1e3


def test_golden_features_are_the_oracles(oracle_run):
    """tests/golden/fid_golden.npz (make_fid_golden.py) against a live oracle run on its first two images."""
    _, taps = oracle_run
    g = np.load(GOLDEN)
    assert tuple(g["hw"]) == fid_util.METRIC_HW and g["f64"].shape == (48, 64) and g["f2048"].shape == (48, 2048)
    for t in (64, 2048):
        want = torch.from_numpy(g[f"f{t}"][:2]).double()
        rel = float((taps[t].double() - want).norm() / want.norm())
        assert rel < 1e-5, (t, rel)              # fp32 conv summation order of the host library; 300x below the gates


# ---- metric state -------------------------------------------------------------------------------------------------------

def _stub_metric(weights_file, **kw):
    m = metrics_registry["fid"](feature=64, weights=weights_file, **kw)
    mix = torch.randn(3, 64, generator=torch.Generator().manual_seed(0))
    m.feature_fn = lambda imgs: torch.relu(imgs.float().mean((2, 3)) / 64.0 @ mix + 0.5)     # host features: no GPU
    return m


def test_metric_state_logic_with_a_stub(weights_file):
    real = fid_util.seeded_images(12, 8, 8, 1)
    gen = fid_util.noisy_copies(real, noise=60)
    m = _stub_metric(weights_file)
    with pytest.raises(RuntimeError, match="More than one sample"):
        m.compute()
    m.update(real, real=True)
    with pytest.raises(RuntimeError, match="More than one sample"):
        m.compute()                                            # nothing on the generated side
    m.update(gen[0], real=False)                               # a 3-D tensor is one image
    with pytest.raises(RuntimeError, match="More than one sample"):
        m.compute()
    m.update(gen[1:6], real=False)
    m.update(gen[6:], real=False)
    v = float(m.compute())
    # the same from the features at once
    from sonicdiffusionbayeslab_amd.fid import frechet_distance
    fr, fg = m.feature_fn(real).double(), m.feature_fn(gen).double()
    want = float(frechet_distance(fr.mean(0), torch.cov(fr.t()), fg.mean(0), torch.cov(fg.t())))
    # (rank-deficient covariances, N = 12 < D = 64: the square roots of the zero eigenvalues carry ~1e-8; gate as for sqrtm)
    assert v > 0 and abs(v - want) <= 1e-6 * want
    m.reset()                                                  # reset_real_features=True: both sides go
    assert m._state["real"] is None and m._state["fake"] is None
    with pytest.raises(RuntimeError):
        m.compute()

    k = _stub_metric(weights_file, reset_real_features=False)
    k.update(real, real=True)
    k.update(gen, real=False)
    first = float(k.compute())
    k.reset()                                                  # keeps the real statistics
    assert k._state["real"] is not None and int(k._state["real"][2]) == 12 and k._state["fake"] is None
    with pytest.raises(RuntimeError):
        k.compute()
    k.update(gen, real=False)
    assert abs(float(k.compute()) - first) <= 1e-12 * first
    assert abs(first - v) <= 1e-6 * v


def test_metric_input_conversion(weights_file):
    real = fid_util.seeded_images(4, 8, 8, 1)
    a = _stub_metric(weights_file)
    b = _stub_metric(weights_file, normalize=True)
    seen = []
    a.feature_fn = b.feature_fn = lambda imgs: seen.append(imgs) or torch.zeros(imgs.shape[0], 64)
    a.update(real, real=True)
    b.update(real.float() / 255.0 + 1e-4, real=True)           # (imgs * 255).byte(): truncation back to the same bytes
    assert seen[0].dtype == torch.uint8 and torch.equal(seen[0], seen[1])
    with pytest.raises(ValueError):
        a.update(real.float(), real=True)                      # float input needs normalize=True


def test_validate_reports_null_fid_without_the_key():
    """A config without quality_metrics.fid.weights: setup_metrics builds no FID metric and says why."""
    from sonicdiffusionbayeslab_amd.experiments.base_experiment import BaseMethod

    class Cfg(dict):
        __getattr__ = dict.get

    class Probe(BaseMethod):
        def __init__(self, cfg):
            self.config, self.device = cfg, "cpu"

        def run_experiment(self):
            pass

    p = Probe(Cfg(quality_metrics=Cfg(clip_score=Cfg(model_name_or_path="openai/clip-vit-base-patch16"))))
    p.setup_metrics()
    assert p.fid_metric is None and p.fid_source == "not configured"
    assert p.fid([torch.zeros(3, 8, 8)], ["a.png"]) is None
    q = Probe(Cfg(quality_metrics=Cfg(fid=Cfg(feature=64, input_img_size=[3, 299, 299], normalize=False, weights="/no/such/file.pth"))))
    q.setup_metrics()
    assert q.fid_metric is None and "not a local file" in q.fid_source
