"""CLIP score of a folder of images against their prompts (the reference's ``calc_clip_score.py`` CLI).

    python calc_clip_score.py --folder_path DIR --prompts_file img2annotations.json \\
        --model_name_or_path LOCAL_CLIP_DIR [--batch_size 32] [--backend hip|transformers]

``--prompts_file`` maps an image file name to its prompt (``data/dataset/img2annotations_test.json``); images of the
folder without a prompt are skipped.  ``--model_name_or_path`` must be a local CLIPModel directory (``config.json``,
``model.safetensors``, ``vocab.json``, ``merges.txt``).  ``--backend hip`` (the default) runs both CLIP towers on libsdhip,
``transformers`` the host path of ``ClipScoreMetric``.

Difference from the reference: the reference loads the images with torchvision's ``ToTensor()`` and hands those [0, 1]
floats to torchmetrics' ``CLIPScore``.  This CLI reads the images as uint8 RGB, as the experiments score their decoded
images (``BaseMethod.clip_score``), and does not reproduce the float path.  Images of the same size are batched
together.  Prints one JSON line with the mean score and the image count.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def load_pairs(folder_path: str, prompts_file: str):
    """``[(file name, uint8 [3,H,W] tensor, prompt)]`` in sorted file-name order."""
    import numpy as np
    import torch
    from PIL import Image
    with open(prompts_file, encoding="utf-8") as f:
        prompts = json.load(f)
    out = []
    for name in sorted(os.listdir(folder_path)):
        if name not in prompts:
            continue
        with Image.open(os.path.join(folder_path, name)) as im:
            arr = np.asarray(im.convert("RGB"), dtype=np.uint8)
        out.append((name, torch.from_numpy(arr.copy()).permute(2, 0, 1).contiguous(), prompts[name]))
    return out


def calc_clip_score(pairs, model_name_or_path: str, batch_size: int = 32, backend: str = "hip") -> float:
    import torch
    from sonicdiffusionbayeslab_amd.metrics import ClipScoreMetric
    metric = ClipScoreMetric(model_name_or_path=model_name_or_path, backend=backend)
    groups = {}
    for _, img, prompt in pairs:
        groups.setdefault(tuple(img.shape), []).append((img, prompt))
    for items in groups.values():
        for s in range(0, len(items), batch_size):
            chunk = items[s:s + batch_size]
            metric.update(torch.stack([i for i, _ in chunk]), [p for _, p in chunk])
    return float(metric.compute())


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description="Calculate CLIP score for images and prompts")
    ap.add_argument("--folder_path", type=str, help="Path to folder containing images")
    ap.add_argument("--prompts_file", type=str, help="JSON file mapping image file names to prompts")
    ap.add_argument("--batch_size", type=int, default=32, help="Batch size for processing")
    ap.add_argument("--model_name_or_path", type=str, default="openai/clip-vit-base-patch16",
                    help="local CLIP model directory")
    ap.add_argument("--backend", type=str, default="hip", choices=("hip", "transformers"))
    args = ap.parse_args(argv)
    if not args.folder_path or not os.path.isdir(args.folder_path):
        raise ValueError("Please provide a valid folder path containing images")
    if not args.prompts_file or not os.path.isfile(args.prompts_file):
        raise ValueError("Please provide a valid JSON file containing prompts")
    pairs = load_pairs(args.folder_path, args.prompts_file)
    if not pairs:
        raise ValueError("no image of the folder has a prompt in the prompts file")
    score = calc_clip_score(pairs, args.model_name_or_path, args.batch_size, args.backend)
    print(json.dumps({"clip_score": score, "images": len(pairs), "backend": args.backend,
                      "model": args.model_name_or_path}), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
