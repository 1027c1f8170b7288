"""FID on libsdhip: the general conv kernel, the pools, the global mean, the preprocessing and sd_fid_accumulate per
element; the Inception features of all four taps against the fp32 oracle; the metric end to end; the validate / CLI wiring.

Gates of the feature and metric tests are reference against reference (tests/golden/make_fid_golden.py prints them; no
kernel takes part): the oracle's bf16-emulating run (every conv input, weight and output rounded to bf16) against its fp32
run, on the seeded weights and images of tests/fid_util.py, times two for a summation order that differs from the host's.

    rel-L2 of the features, 4 images 512 x 512:   e_tap = 1.4998e-03 (64), 1.9050e-03 (192), 3.6006e-03 (768), 4.1154e-03 (2048)
    relative gap of the FID, 24 + 24 images:      e_fid = 5.5593e-04 (feature 64), 4.4634e-03 (feature 2048)
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from sonicdiffusionbayeslab_amd import _lib
from tests import fid_util, inception_oracle
from tests.bounds import ATOL_TINY, U32, assert_elementwise, check_guards, guarded, guarded_input, linear_bound, ulp_bf16
from tests.util import rel_l2

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_TAP = {64: 1.4998e-03, 192: 1.9050e-03, 768: 3.6006e-03, 2048: 4.1154e-03}
E_FID = {64: 5.5593e-04, 2048: 4.4634e-03}
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fid_golden.npz")


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


# ---- conv ---------------------------------------------------------------------------------------------------------------
# (B, side_h, side_w, Cin, Cout, kh, kw, stride, ph, pw): one case of every (kernel, stride, padding) of the network at the
# table's awkward channel counts and sides, and one with nothing a multiple of anything (element-load path, K and Cout tails)
CONV_CASES = [
    (1, 299, 299, 3, 32, 3, 3, 2, 0, 0),       # Conv2d_1a: Cin 3 (element loads), K = 27 < one step, 149 x 149 rows
    (1, 73, 73, 80, 192, 3, 3, 1, 0, 0),       # Conv2d_4a
    (2, 35, 35, 48, 64, 5, 5, 1, 2, 2),        # branch5x5_2: K = 1200 = 37.5 steps
    (2, 35, 35, 288, 384, 3, 3, 2, 0, 0),      # Mixed_6a.branch3x3
    (2, 17, 17, 160, 160, 1, 7, 1, 0, 3),
    (2, 17, 17, 160, 160, 7, 1, 1, 3, 0),
    (3, 8, 8, 448, 384, 3, 3, 1, 1, 1),        # Mixed_7b/c.branch3x3dbl_2
    (3, 8, 8, 1280, 320, 1, 1, 1, 0, 0),       # Mixed_7b.branch1x1: 192 rows = 3 row tiles
    (2, 8, 8, 384, 384, 1, 3, 1, 0, 1),
    (2, 8, 8, 384, 384, 3, 1, 1, 1, 0),
    (2, 9, 11, 13, 70, 3, 3, 1, 1, 1),         # odd everything
    (1, 5, 7, 24, 8, 3, 3, 2, 1, 1),           # fewer rows and columns than one tile
]


@pytest.mark.parametrize("case", CONV_CASES, ids=lambda c: "x".join(str(v) for v in c))
def test_conv_per_element(sdlib, case):
    B, H, W, Cin, Cout, kh, kw, stride, ph, pw = case
    g = torch.Generator().manual_seed(sum(case))
    x = torch.randn(B, Cin, H, W, generator=g).bfloat16()
    w = (torch.randn(Cout, Cin, kh, kw, generator=g) * (2.0 / (Cin * kh * kw)) ** 0.5).bfloat16()
    bias = 0.2 * torch.randn(Cout, generator=g)
    pre = F.conv2d(x.double(), w.double(), bias.double(), stride=stride, padding=(ph, pw))
    mag = F.conv2d(x.double().abs(), w.double().abs(), bias.double().abs(), stride=stride, padding=(ph, pw))
    Ho, Wo = pre.shape[2:]
    odd = Cin % 8 != 0
    coff, ldy = (5, Cout + 11) if odd else (8, Cout + 24)
    xd = guarded_input(_nhwc(x).reshape(B * H * W, Cin), label="x")
    wd = guarded_input(_nhwc(w).reshape(Cout, kh * kw * Cin), label="w")
    bd = guarded_input(bias.view(1, Cout), label="bias")
    for relu in (1, 0):
        y = guarded((B * Ho * Wo, coff + Cout), torch.bfloat16, ld=ldy, label="y")
        _lib.check(sdlib.sd_op_inception_conv(_lib.current_stream(), xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), y.data_ptr(), B, H, W,
                                              Cin, Cout, kh, kw, stride, ph, pw, ldy, coff, relu), "sd_op_inception_conv")
        torch.cuda.synchronize()
        out = y.cpu()
        assert torch.isnan(out[:, :coff]).all(), "channels before the slice were written"
        ref = _nhwc(torch.relu(pre) if relu else pre).reshape(B * Ho * Wo, Cout)
        bound = linear_bound(ref, _nhwc(mag).reshape(B * Ho * Wo, Cout), kh * kw * Cin + 2)
        assert_elementwise(out[:, coff:].float(), ref, bound, f"inception conv {case} relu={relu}", names=("row", "c"))
    check_guards()


def test_conv_rejects_bad_arguments(sdlib):
    t = torch.zeros(4096, dtype=torch.bfloat16, device="cuda")
    s = _lib.current_stream()
    with pytest.raises(_lib.SdHipError, match="pitch"):
        _lib.check(sdlib.sd_op_inception_conv(s, t.data_ptr(), t.data_ptr(), None, t.data_ptr(), 1, 4, 4, 8, 8, 1, 1, 1, 0, 0, 12, 8, 1))
    with pytest.raises(_lib.SdHipError, match="larger than"):
        _lib.check(sdlib.sd_op_inception_conv(s, t.data_ptr(), t.data_ptr(), None, t.data_ptr(), 1, 2, 2, 8, 8, 3, 3, 1, 0, 0, 8, 0, 1))


# ---- pools and the mean -------------------------------------------------------------------------------------------------
# (B, H, W, C, stride, pad, ldy, coff)
MAXPOOL_CASES = [(1, 147, 147, 64, 2, 0, 64, 0), (2, 35, 35, 288, 2, 0, 768, 480), (2, 8, 8, 2048, 1, 1, 2048, 0),
                 (2, 17, 17, 768, 2, 0, 1280, 512), (2, 9, 11, 13, 2, 0, 21, 3), (2, 7, 5, 13, 1, 1, 13, 0), (1, 3, 3, 8, 2, 0, 8, 0)]


@pytest.mark.parametrize("case", MAXPOOL_CASES, ids=lambda c: "x".join(str(v) for v in c))
def test_maxpool_exact(sdlib, case):
    B, H, W, C, stride, pad, ldy, coff = case
    x = torch.randn(B, C, H, W, generator=torch.Generator().manual_seed(sum(case))).bfloat16()
    ref = _nhwc(F.max_pool2d(x.float(), 3, stride=stride, padding=pad))
    Ho, Wo = ref.shape[1:3]
    xd = guarded_input(_nhwc(x).reshape(B * H * W, C), label="x")
    y = guarded((B * Ho * Wo, coff + C), torch.bfloat16, ld=ldy, label="y")
    _lib.check(sdlib.sd_op_maxpool3x3(_lib.current_stream(), xd.data_ptr(), y.data_ptr(), B, H, W, C, stride, pad, ldy, coff),
               "sd_op_maxpool3x3")
    torch.cuda.synchronize()
    out = y.cpu()
    assert torch.isnan(out[:, :coff]).all()
    assert torch.equal(out[:, coff:].float(), ref.reshape(-1, C))
    check_guards()


AVGPOOL_CASES = [(2, 35, 35, 192, 192, 0), (2, 17, 17, 768, 776, 8), (2, 8, 8, 1280, 1280, 0), (2, 7, 5, 13, 20, 3),
                 (1, 1, 1, 8, 8, 0), (1, 2, 3, 16, 16, 0)]


@pytest.mark.parametrize("case", AVGPOOL_CASES, ids=lambda c: "x".join(str(v) for v in c))
def test_avgpool_per_element(sdlib, case):
    """Edge and corner pixels divide by 6 and 4 (count_include_pad=False); one bf16 ulp + 10 fp32 roundings (8 additions, the
    division, slack of one) on the magnitude."""
    B, H, W, C, ldy, coff = case
    x = torch.randn(B, C, H, W, generator=torch.Generator().manual_seed(sum(case))).bfloat16()
    ref = _nhwc(F.avg_pool2d(x.double(), 3, stride=1, padding=1, count_include_pad=False)).reshape(-1, C)
    mag = _nhwc(F.avg_pool2d(x.double().abs(), 3, stride=1, padding=1, count_include_pad=False)).reshape(-1, C)
    xd = guarded_input(_nhwc(x).reshape(B * H * W, C), label="x")
    y = guarded((B * H * W, coff + C), torch.bfloat16, ld=ldy, label="y")
    _lib.check(sdlib.sd_op_avgpool3x3(_lib.current_stream(), xd.data_ptr(), y.data_ptr(), B, H, W, C, ldy, coff), "sd_op_avgpool3x3")
    torch.cuda.synchronize()
    out = y.cpu()
    assert torch.isnan(out[:, :coff]).all()
    assert_elementwise(out[:, coff:].float(), ref, ulp_bf16(ref) + 10 * U32 * mag + ATOL_TINY, f"avgpool {case}", names=("row", "c"))
    check_guards()


@pytest.mark.parametrize("B,HW,C", [(2, 73 * 73, 64), (2, 35 * 35, 192), (2, 17 * 17, 768), (3, 64, 2048), (2, 7, 13), (1, 1, 70)])
def test_global_mean_per_element(sdlib, B, HW, C):
    x = (torch.randn(B, HW, C, generator=torch.Generator().manual_seed(HW + C)) + 0.5).bfloat16()
    xd = guarded_input(x.reshape(B * HW, C), label="x")
    out = guarded((B, C), torch.float32, label="mean")
    _lib.check(sdlib.sd_op_global_mean(_lib.current_stream(), xd.data_ptr(), out.data_ptr(), B, HW, C), "sd_op_global_mean")
    torch.cuda.synchronize()
    ref, mag = x.double().mean(1), x.double().abs().mean(1)
    assert_elementwise(out.cpu(), ref, (HW + 2) * U32 * mag + ATOL_TINY, f"global mean {B}x{HW}x{C}", names=("b", "c"))
    check_guards()


# ---- preprocessing ------------------------------------------------------------------------------------------------------
RESIZE_SIZES = [(512, 512), (512, 768), (1024, 1024), (299, 299), (100, 150), (37, 53), (1, 1)]


@pytest.mark.parametrize("h,w", RESIZE_SIZES)
def test_resize_per_element(sdlib, h, w):
    B, S = 2, 299
    imgs = torch.randint(0, 256, (B, 3, h, w), generator=torch.Generator().manual_seed(h * 31 + w), dtype=torch.uint8)
    ref = _nhwc(inception_oracle.preprocess(imgs)).double().reshape(B * S * S, 3)
    xd = guarded_input(imgs.reshape(B * 3 * h, w), label="images")
    o32 = guarded((B * S * S, 3), torch.float32, label="fp32 out")
    o16 = guarded((B * S * S, 3), torch.bfloat16, label="bf16 out")
    for o, flag in ((o32, 1), (o16, 0)):
        _lib.check(sdlib.sd_op_inception_resize(_lib.current_stream(), xd.data_ptr(), B, h, w, o.data_ptr(), flag), "sd_op_inception_resize")
    torch.cuda.synchronize()
    b32 = 8 * U32 * ref.abs().clamp(min=1.0)
    assert_elementwise(o32.cpu(), ref, b32, f"resize {h}x{w} fp32", names=("pixel", "c"))
    assert_elementwise(o16.cpu().float(), ref, b32 + ulp_bf16(ref), f"resize {h}x{w} bf16", names=("pixel", "c"))
    check_guards()


# ---- statistics ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("D", [64, 200])
def test_fid_accumulate_per_element(D):
    from sonicdiffusionbayeslab_amd.fid import fid_accumulate
    g = torch.Generator().manual_seed(D)
    total = torch.zeros(D, dtype=torch.float64, device="cuda")
    cov = torch.zeros(D, D, dtype=torch.float64, device="cuda")
    count = torch.zeros(1, dtype=torch.int64, device="cuda")
    seen = []
    for B in (5, 3):
        f = torch.relu(torch.randn(B, D, generator=g) + 0.3) * 3.0
        seen.append(f)
        fid_accumulate(f.cuda(), total, cov, count)
        torch.cuda.synchronize()
        a = torch.cat(seen).double().numpy()
        n = a.shape[0]
        assert int(count.item()) == n
        assert_elementwise(total.cpu(), torch.from_numpy(a.sum(0)), (n + 2) * 2.0 ** -53 * torch.from_numpy(np.abs(a).sum(0)) + ATOL_TINY,
                           f"fid sum D={D} after {n}", names=("j",))
        assert_elementwise(cov.cpu(), torch.from_numpy(a.T @ a), (n + 2) * 2.0 ** -53 * torch.from_numpy(np.abs(a).T @ np.abs(a)) + ATOL_TINY,
                           f"fid cov_sum D={D} after {n}", names=("i", "j"))


# ---- the network --------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def state_dict():
    return fid_util.random_state_dict(0)


@pytest.fixture(scope="module")
def net(state_dict):
    from sonicdiffusionbayeslab_amd.fid import HipInceptionFeatures
    return HipInceptionFeatures.from_state_dict(state_dict)


@pytest.fixture(scope="module")
def feature_reference(state_dict):
    imgs = fid_util.seeded_images(4, 512, 512, 0)
    return imgs, inception_oracle.inception_features(state_dict, imgs)


@pytest.mark.parametrize("tap", [64, 192, 768, 2048])
def test_features_against_fp32_oracle(net, feature_reference, tap):
    imgs, ref = feature_reference
    got = net.features(imgs, tap).cpu()
    assert got.shape == (4, tap) and got.dtype == torch.float32 and torch.isfinite(got).all()
    err = rel_l2(got, ref[tap])
    print(f"[fid] tap {tap}: rel-L2 against the fp32 oracle {err:.4e}; e_tap {E_TAP[tap]:.4e}, gate {2 * E_TAP[tap]:.4e}")
    assert err <= 2 * E_TAP[tap]
    # a sample's features do not depend on the batch it is in
    assert torch.equal(net.features(imgs[1:2], tap).cpu(), got[1:2])


def test_features_take_any_input_size_and_reject_bad_taps(net, state_dict):
    imgs = fid_util.seeded_images(3, 100, 150, 4)
    ref = inception_oracle.inception_features(state_dict, imgs, upto=192)
    for tap in (64, 192):
        err = rel_l2(net.features(imgs, tap).cpu(), ref[tap])
        print(f"[fid] 100x150 tap {tap}: rel-L2 {err:.4e}")
        assert err <= 2 * E_TAP[tap]
    with pytest.raises(ValueError, match="64, 192, 768, 2048"):
        net.features(imgs, 1000)
    with pytest.raises(ValueError):
        net.features(imgs.float(), 64)


# ---- the metric ---------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def weights_file(tmp_path_factory, state_dict):
    p = tmp_path_factory.mktemp("fid") / "inception.pth"
    torch.save(state_dict, str(p))
    return str(p)


def _fid_from_features(f, n):
    from sonicdiffusionbayeslab_amd.fid import frechet_distance
    r, q = f[:n].double(), f[n:].double()
    return float(frechet_distance(r.mean(0), torch.cov(r.t()), q.mean(0), torch.cov(q.t())))


@pytest.mark.parametrize("feature", [64, 2048])
def test_metric_end_to_end(weights_file, feature):
    """24 real and 24 generated (gain + noise) images through the metric on the GPU, against the FID of the fp32 oracle's
    features of the same images (tests/golden/fid_golden.npz).  Gate: 2 e_fid, e_fid = the oracle's own bf16-emulating FID
    against its fp32 FID (module docstring).  FID(real, real) < 1e-6 FID(real, generated), as a signed comparison: with 24
    samples the covariances are rank-deficient and the fp64 eigenvalue solver leaves a residue of either sign (measured
    -3.1e-08 of FID(real, generated) at feature 64 and -1.4e-06 at 2048; the oracle's own features give -7.8e-07 at 2048 on
    the host), so the magnitude at 2048 is the host solver's, not the kernels'."""
    from sonicdiffusionbayeslab_amd.metrics import FID
    real, gen = fid_util.metric_images()
    n = real.shape[0]
    want = _fid_from_features(torch.from_numpy(np.load(GOLDEN)[f"f{feature}"]), n)
    m = FID(feature=feature, weights=weights_file, reset_real_features=False)
    for s in range(0, n, 8):
        m.update(real[s:s + 8], real=True)
        m.update(gen[s:s + 8], real=False)
    got = float(m.compute())
    gap = abs(got - want) / want
    m.reset()                                   # keeps the real side
    m.update(real[:16], real=False)
    m.update(real[16:], real=False)
    same = float(m.compute())
    print(f"[fid] feature {feature}: GPU {got:.8g}, fp32 oracle {want:.8g}, relative gap {gap:.4e}; e_fid {E_FID[feature]:.4e}, "
          f"gate {2 * E_FID[feature]:.4e}; FID(real, real) {same:.3e} = {same / got:.3e} of FID(real, generated)")
    assert gap <= 2 * E_FID[feature]
    assert same < 1e-6 * got


# ---- wiring -------------------------------------------------------------------------------------------------------------

def _write_images(folder, images, names=None):
    from PIL import Image
    os.makedirs(folder, exist_ok=True)
    names = names or [f"{i:03d}.png" for i in range(len(images))]
    for name, im in zip(names, images):
        Image.fromarray(im.permute(1, 2, 0).numpy(), "RGB").save(os.path.join(folder, name))
    return names


def test_validate_reports_fid(weights_file, tmp_path, capsys):
    from sonicdiffusionbayeslab_amd.config import _wrap
    from sonicdiffusionbayeslab_amd.experiments.base_experiment import BaseMethod
    from sonicdiffusionbayeslab_amd.metrics import FID
    from sonicdiffusionbayeslab_amd.weights import UNetConfig
    prompts = json.load(open(os.path.join(ROOT, "data", "dataset", "img2annotations_test.json")))
    names = sorted(prompts)[:4]
    img_dir = str(tmp_path / "imgs")
    _write_images(img_dir, fid_util.seeded_images(4, 64, 64, 11), names)
    pf = tmp_path / "prompts.json"
    pf.write_text(json.dumps({k: prompts[k] for k in names}))
    decoded = []

    class _Stub:            # a pipeline that "decodes" seeded images in [0, 1]
        weights_source, num_timesteps = "stub", 2

        def __init__(self):
            self.unet_config = UNetConfig(sample_size=8)
            self.scheduler = type("S", (), {"config": {}})()

        def to(self, device):
            return self

        def __call__(self, prompts, generator=None, output_type="pt", **kw):
            imgs = torch.rand((len(prompts), 3, 64, 64), generator=generator)
            decoded.extend(imgs)
            return type("O", (), {"images": imgs})(), 0.1, []

    class M(BaseMethod):
        def setup_model(self):
            self.model = _Stub()

        def setup_scheduler(self, **kw):
            pass

        def run_experiment(self):
            self.sweep([2], lambda n: {"num_inference_steps": n}, lambda n: f"steps {n}")

    base = {"experiment_name": "stub", "experiment": {"method": "stub", "seed": 29},
            "dataset": {"img_dataset": img_dir, "prompts": str(pf), "image_size": 64},
            "inference": {"batch_size": 4, "batch_count": 1}}
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "SD_DIST_FORCE_INIT"):
        os.environ.pop(k, None)
    with_fid = dict(base, quality_metrics={"fid": {"feature": 64, "input_img_size": [3, 299, 299], "normalize": False,
                                                   "weights": weights_file}})
    m = M(_wrap(with_fid))
    assert m.fid_metric is not None and m.fid_metric.feature_fn is None
    m.run_experiment()
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    ref = FID(feature=64, weights=weights_file)
    ref.update((torch.stack(decoded) * 255).to(torch.uint8), real=False)
    ref.update((m.load_images(m.last_image_files) * 255).to(torch.uint8), real=True)
    print(f"validate fid: {line['fid']:.6g}, the metric alone {float(ref.compute()):.6g}")
    assert line["images"] == 4 and line["fid_weights"] == weights_file
    assert np.isfinite(line["fid"]) and line["fid"] > 0 and line["fid"] == float(ref.compute())
    assert m.metric_dict["fid"] == [line["fid"]]
    # without the key: null, a reason, and the fields a run had before
    del decoded[:]
    k = M(_wrap(base))
    assert k.fid_metric is None
    k.run_experiment()
    line2 = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert line2["fid"] is None and line2["fid_weights"] == "not configured" and "fid" not in k.metric_dict
    before = ["experiment", "run", "nfe", "images", "time_metric_s_per_image", "images_per_s", "weights", "clip_score",
              "clip_score_model", "n_gpus", "fp8_activation_scales"]
    assert list(line2)[:len(before)] == before and set(line2) - set(before) == {"fid", "fid_weights"}
    assert line2["clip_score"] is None and line2["images"] == 4 and line2["nfe"] == 2


def test_calc_fid_cli(weights_file, tmp_path):
    real = fid_util.seeded_images(6, 48, 64, 21)
    _write_images(str(tmp_path / "real"), real)
    _write_images(str(tmp_path / "gen"), fid_util.noisy_copies(real))
    r = subprocess.run(["timeout", "-k", "10", "240", sys.executable, os.path.join(ROOT, "calc_fid.py"), str(tmp_path / "real"),
                        str(tmp_path / "gen"), "--weights", weights_file, "--feature", "192", "--batch-size", "4"],
                       capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    print(f"calc_fid.py: {res}")
    assert res["n_real"] == 6 and res["n_gen"] == 6 and res["feature"] == 192
    assert np.isfinite(res["fid"]) and res["fid"] > 0 and res["images_per_s"] > 0
