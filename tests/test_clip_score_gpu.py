"""CLIP score on libsdhip: the preprocessing kernel against Pillow (bit-exact uint8 crop), the ViT attention kernel per
element, the tiny CLIP against the committed transformers goldens, the full-size ViT-B/16 and ViT-L/14 vision shapes
against the fp32 oracle, and the metric / validate / CLI wiring."""
import json
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

from sonicdiffusionbayeslab_amd import _lib
from tests.bounds import attention_elementwise, check_guards, guarded, guarded_input
from tests.clip_score_util import PROMPTS, tiny_configs, tiny_images, tiny_state_dict, write_tiny_clip_dir
from tests.clip_vision_oracle import clip_scores, clip_text_embeds, clip_vision_forward, pil_crop, pixel_values
from tests.util import rel_l2

TOL = 1.5e-2           # the text tower's gate (tests/test_clip_gpu.py)
SCORE_TOL = 0.5        # per-pair 100 cos, absolute
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "clip_score_golden.json")))
PREP_SIZES = [(512, 512), (512, 768), (768, 512), (1024, 1024), (224, 224), (100, 150), (37, 53), (1, 1)]


@pytest.mark.parametrize("h,w", PREP_SIZES)
def test_preprocess_crop_equals_pil(sdlib, h, w):
    B, S, P = 3, 224, 14              # ViT-L/14: K = 588 padded to 640
    g = torch.Generator().manual_seed(h * 31 + w)
    imgs = torch.randint(0, 256, (B, 3, h, w), generator=g, dtype=torch.uint8)
    x = guarded_input(imgs.reshape(B * 3 * h, w), label="images")
    crop = guarded((B * 3 * S, S), torch.uint8, fill=None, label="crop")
    Kp, Np = 640, (S // P) ** 2
    patches = guarded((B * Np, Kp), torch.bfloat16, label="patches")
    _lib.check(sdlib.sd_op_clip_preprocess(_lib.current_stream(), x.data_ptr(), B, h, w, S, P, crop.data_ptr(),
                                           patches.data_ptr()), "sd_op_clip_preprocess")
    torch.cuda.synchronize()
    got = crop.cpu().reshape(B, 3, S, S)
    pt = patches.float().cpu()
    check_guards()
    for b in range(B):
        want = pil_crop(imgs[b], S)
        assert torch.equal(got[b], want), f"{h}x{w} image {b}: {(got[b] != want).sum().item()} pixels differ"
        pix = pixel_values(want)                                                   # [3, S, S]
        rows = pix.reshape(3, S // P, P, S // P, P).permute(1, 3, 0, 2, 4).reshape(Np, 3 * P * P)
        ref = rows.to(torch.bfloat16).float()
        assert torch.equal(pt[b * Np:(b + 1) * Np, :3 * P * P], ref)
    assert (pt[:, 3 * P * P:] == 0).all()


@pytest.mark.parametrize("L", [1, 17, 50, 63, 65, 197, 257, 320])
def test_vit_attention_per_element(sdlib, L):
    for B, heads in ((1, 1), (2, 3), (3, 2)):
        H = 64 * heads
        g = torch.Generator().manual_seed(L * 100 + B * 10 + heads)
        qkv = (torch.randn(B * L, 3 * H, generator=g) * 1.5).to(torch.bfloat16)
        x = guarded_input(qkv, label="qkv")
        out = guarded((B * L, H), torch.bfloat16, label="out")
        _lib.check(sdlib.sd_op_vit_attention(_lib.current_stream(), x.data_ptr(), out.data_ptr(), B, L, H, heads),
                   "sd_op_vit_attention")
        torch.cuda.synchronize()
        q, k, v = (qkv[:, i * H:(i + 1) * H].float().view(B, L, H) for i in range(3))
        attention_elementwise(out.cpu().float().view(B, L, H), q, k, v, heads, 64, f"vit attention L={L} B={B} heads={heads}")
        check_guards()
    with pytest.raises(_lib.SdHipError):
        _lib.check(sdlib.sd_op_vit_attention(_lib.current_stream(), x.data_ptr(), out.data_ptr(), 1, 321, 64, 1))


@pytest.fixture(scope="module")
def tiny_dir(tmp_path_factory):
    return write_tiny_clip_dir(str(tmp_path_factory.mktemp("clip") / "tiny"))


def test_tiny_clip_matches_transformers_goldens(tiny_dir):
    from sonicdiffusionbayeslab_amd.clip_score import HipClipScorer
    sc = HipClipScorer.from_pretrained(tiny_dir)
    images = tiny_images()
    img = sc.image_embeds(images).cpu()
    txt = sc.text_embeds(PROMPTS).cpu()
    gi, gt = torch.tensor(GOLD["image_embeds"]), torch.tensor(GOLD["text_embeds"])
    raw, score = sc.score_pairs(images, PROMPTS)
    raw, score = raw.cpu(), score.cpu()
    graw = torch.tensor(GOLD["raw_scores"])
    # the oracle on the same weights (sanity of the golden itself)
    tcfg, vcfg = tiny_configs()
    sd = tiny_state_dict()
    oi = clip_vision_forward(sd, vcfg, torch.stack([pixel_values(pil_crop(im, 224)) for im in images]))
    ot = clip_text_embeds(sd, tcfg, sc.tokenizer(PROMPTS), None)
    print(f"tiny CLIP vs transformers: image embeds rel-L2 {rel_l2(img, gi):.3e}, text embeds {rel_l2(txt, gt):.3e}, "
          f"max |d raw score| {(raw - graw).abs().max().item():.4f}; vs oracle: image {rel_l2(img, oi):.3e} "
          f"text {rel_l2(txt, ot):.3e}")
    for i in range(len(images)):
        print(f"  pair {i} {tuple(images[i].shape[1:])}: raw {raw[i].item():+.4f} transformers {graw[i].item():+.4f}")
    assert rel_l2(img, gi) <= TOL and rel_l2(txt, gt) <= TOL
    assert (raw - graw).abs().max().item() <= SCORE_TOL
    assert torch.equal(score, raw.clamp(min=0))
    assert rel_l2(img, oi) <= TOL and rel_l2(txt, ot) <= TOL


def test_metric_hip_backend_mean_matches_transformers(tiny_dir):
    from sonicdiffusionbayeslab_amd.metrics import ClipScoreMetric
    m = ClipScoreMetric(tiny_dir, backend="hip")
    images = tiny_images()
    m.update(images, PROMPTS)                       # a list of mixed sizes: grouped by size inside
    mean = float(m.compute())
    print(f"metric mean: hip {mean:.4f}, transformers golden {GOLD['metric_mean']:.4f}")
    assert abs(mean - GOLD["metric_mean"]) <= SCORE_TOL
    m.reset()
    for s in range(0, len(images), 2):
        m.update(torch.stack(images[s:s + 2]), PROMPTS[s:s + 2])
    assert abs(float(m.compute()) - mean) < 1e-3


@pytest.mark.parametrize("shape", ["B/16", "L/14"])
def test_full_size_vision_towers_against_oracle(shape):
    from sonicdiffusionbayeslab_amd.clip_score import (ClipVisionConfig, HipClipVisionModel,
                                                       make_synthetic_clip_vision_state_dict)
    cfg = ClipVisionConfig() if shape == "B/16" else ClipVisionConfig(hidden_size=1024, num_hidden_layers=24,
                                                                      num_attention_heads=16, intermediate_size=4096,
                                                                      patch_size=14, projection_dim=768)
    sd = make_synthetic_clip_vision_state_dict(cfg, seed=99)
    m = HipClipVisionModel(cfg, sd)
    g = torch.Generator().manual_seed(5)
    for h, w in ((512, 512), (512, 768)):
        imgs = torch.randint(0, 256, (2, 3, h, w), generator=g, dtype=torch.uint8)
        got = m.encode(imgs).cpu()
        ref = clip_vision_forward(sd, cfg, torch.stack([pixel_values(pil_crop(i, 224)) for i in imgs]))
        err = rel_l2(got, ref)
        d = (clip_scores(got, ref) - 100).abs().max().item()
        print(f"ViT-{shape} {h}x{w}: image embeds rel-L2 {err:.3e}, max 100(1 - cos) {d:.4f}")
        assert err <= TOL and d <= SCORE_TOL


def test_validate_reports_hip_clip_score_and_cli(tiny_dir, tmp_path, capsys):
    """BaseMethod.validate with quality_metrics.clip_score.backend = hip reports clip_score on decoded images; the CLI
    scores a folder written here."""
    from sonicdiffusionbayeslab_amd.config import _wrap
    from sonicdiffusionbayeslab_amd.experiments.base_experiment import BaseMethod
    from sonicdiffusionbayeslab_amd.metrics import ClipScoreMetric
    from sonicdiffusionbayeslab_amd.weights import UNetConfig
    decoded = {}

    class _Stub:            # a pipeline that "decodes" seeded images in [0, 1]
        weights_source, num_timesteps = "stub", 2

        def __init__(self):
            self.unet_config = UNetConfig(sample_size=8)
            self.scheduler = type("S", (), {"config": {}})()

        def to(self, device):
            return self

        def __call__(self, prompts, generator=None, output_type="pt", **kw):
            imgs = torch.rand((len(prompts), 3, 64, 96), generator=generator)
            decoded.setdefault("images", []).extend(imgs)
            decoded.setdefault("prompts", []).extend(prompts)
            return type("O", (), {"images": imgs})(), 0.1, []

    class M(BaseMethod):
        def setup_model(self):
            self.model = _Stub()

        def setup_scheduler(self, **kw):
            pass

        def run_experiment(self):
            self.sweep([2], lambda n: {"num_inference_steps": n}, lambda n: f"steps {n}")

    base = {"experiment_name": "stub", "experiment": {"method": "stub", "seed": 29},
            "dataset": {"img_dataset": "", "prompts": os.path.join(ROOT, "data", "dataset", "img2annotations_test.json")},
            "inference": {"batch_size": 3, "batch_count": 1},
            "quality_metrics": {"clip_score": {"model_name_or_path": tiny_dir, "backend": "hip"}}}
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "SD_DIST_FORCE_INIT"):
        os.environ.pop(k, None)
    m = M(_wrap(base))
    m.device = "cpu"
    assert m.clip_score_gen_metric.backend == "hip"
    m.run_experiment()
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    ref = ClipScoreMetric(tiny_dir, backend="transformers")
    ref.update((torch.stack(decoded["images"]) * 255).to(torch.uint8), decoded["prompts"])
    print(f"validate clip_score: hip {line['clip_score']:.4f}, transformers {float(ref.compute()):.4f}")
    assert line["images"] == 3 and line["clip_score_model"] == tiny_dir
    assert abs(line["clip_score"] - float(ref.compute())) <= SCORE_TOL
    # CLI on a folder
    from PIL import Image
    folder = tmp_path / "imgs"
    folder.mkdir()
    images = tiny_images()[:4]
    prompts = {}
    for i, im in enumerate(images):
        Image.fromarray(im.permute(1, 2, 0).numpy(), "RGB").save(folder / f"{i:03d}.png")
        prompts[f"{i:03d}.png"] = PROMPTS[i]
    pf = tmp_path / "prompts.json"
    pf.write_text(json.dumps(prompts))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "calc_clip_score.py"), "--folder_path", str(folder),
                        "--prompts_file", str(pf), "--model_name_or_path", tiny_dir, "--batch_size", "2"],
                       capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    want = float(torch.tensor(GOLD["raw_scores"][:4]).clamp(min=0).mean())
    print(f"calc_clip_score.py: {res['clip_score']:.4f} over {res['images']} images (transformers golden {want:.4f})")
    assert res["images"] == 4 and res["backend"] == "hip" and abs(res["clip_score"] - want) <= SCORE_TOL


def test_scorer_follows_its_device_and_leaves_the_current_device(tiny_dir, monkeypatch):
    """The hip metric builds its towers on the device it is given, at the first update, and never changes the process's
    current device (a rank pinned to cuda:k keeps launching its UNet on cuda:k).  With two GPUs the towers run on cuda:1
    while cuda:0 is current and give cuda:0's embeddings."""
    from sonicdiffusionbayeslab_amd.metrics import ClipScoreMetric

    def no_set_device(*a, **k):
        raise AssertionError("the CLIP scorer changed the current device")
    images, prompts = tiny_images()[:4], PROMPTS[:4]
    ref = None
    for dev in range(min(torch.cuda.device_count(), 2)):
        torch.cuda.set_device(0)
        with monkeypatch.context() as mp:
            mp.setattr(torch.cuda, "set_device", no_set_device)
            m = ClipScoreMetric(tiny_dir, backend="hip", device=f"cuda:{dev}")
            assert m.scorer is None
            m.update(images, prompts)
            sc = m.scorer
            assert sc.vision_model.device == torch.device("cuda", dev) == sc.text_model.device
            img = sc.image_embeds(images)
            assert img.device == torch.device("cuda", dev)
        assert torch.cuda.current_device() == 0
        print(f"scorer on cuda:{dev}: mean {float(m.compute()):.4f}")
        if ref is None:
            ref = img.cpu()
        else:
            assert torch.equal(img.cpu(), ref)
