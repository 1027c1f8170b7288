"""Writes tests/golden/clip_score_golden.json from the transformers build in this image (third-party library, NOT the
reference): the tiny CLIPModel of tests/clip_score_util.py (seeded weights, written as a local checkpoint directory) scores
the seeded uint8 images against the prompts through ``ClipScoreMetric(backend="transformers")``'s path -- CLIPProcessor
(PIL backend), ``get_image_features`` / ``get_text_features`` -- and the JSON records the image / text embeddings, the
unclamped per-pair ``100 cos`` and the metric's mean.  Run from the repo root:
``python tests/golden/make_clip_score_golden.py``."""
import json
import os
import sys
import tempfile

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from tests.clip_score_util import IMAGE_SIZES, PROMPTS, tiny_images, write_tiny_clip_dir  # noqa: E402


def record(model_dir):
    import transformers
    from sonicdiffusionbayeslab_amd.metrics import ClipScoreMetric
    m = ClipScoreMetric(model_dir, backend="transformers")
    images = tiny_images()
    inp = m.processor(text=PROMPTS, images=images, return_tensors="pt", padding=True, truncation=True)
    emb = lambda o: o if torch.is_tensor(o) else o.pooler_output
    with torch.no_grad():
        img = emb(m.model.get_image_features(pixel_values=inp["pixel_values"]))
        txt = emb(m.model.get_text_features(input_ids=inp["input_ids"], attention_mask=inp["attention_mask"]))
    raw = 100 * ((img / img.norm(dim=-1, keepdim=True)) * (txt / txt.norm(dim=-1, keepdim=True))).sum(-1)
    m.update(torch.stack(images[:2]), PROMPTS[:2])       # the metric itself, on one same-size batch
    for s in range(2, len(images), 2):
        m.update(torch.stack(images[s:s + 2]), PROMPTS[s:s + 2])
    r = lambda t: [[round(float(v), 7) for v in row] for row in t]
    return {"transformers_version": transformers.__version__, "image_sizes": IMAGE_SIZES, "prompts": PROMPTS,
            "input_ids": inp["input_ids"].tolist(), "image_embeds": r(img), "text_embeds": r(txt),
            "raw_scores": [round(float(v), 6) for v in raw], "metric_mean": round(float(m.compute()), 6)}


def main():
    with tempfile.TemporaryDirectory() as d:
        res = record(write_tiny_clip_dir(d))
    path = os.path.join(ROOT, "tests", "golden", "clip_score_golden.json")
    json.dump(res, open(path, "w"))
    print("wrote", path, os.path.getsize(path), "bytes; raw scores", res["raw_scores"], "mean", res["metric_mean"])


if __name__ == "__main__":
    main()
