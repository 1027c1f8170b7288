"""FID between two folders of images on libsdhip (beside ``calc_clip_score.py``).

    python calc_fid.py REAL_DIR GEN_DIR --weights LOCAL_INCEPTION.pth [--feature 2048] [--batch-size 32]

``--weights`` is a local state dict of the FID Inception-v3 (pt_inception-2015-12-05; ``.pth`` or ``.safetensors``).  Every
image file of a folder is read as uint8 RGB at its own size (the network's preprocessing resizes to 299 x 299); images of
the same size are batched together.  Prints one JSON line: ``fid``, ``n_real``, ``n_gen``, ``images_per_s`` (both folders
through the feature extractor, file reading excluded).
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

EXTENSIONS = (".png", ".jpg", ".jpeg", ".bmp", ".webp")


def load_folder(folder: str):
    """uint8 ``[3,H,W]`` tensors of the folder's image files in sorted file-name order."""
    import numpy as np
    import torch
    from PIL import Image
    out = []
    for name in sorted(os.listdir(folder)):
        if not name.lower().endswith(EXTENSIONS):
            continue
        with Image.open(os.path.join(folder, name)) as im:
            arr = np.asarray(im.convert("RGB"), dtype=np.uint8)
        out.append(torch.from_numpy(arr.copy()).permute(2, 0, 1).contiguous())
    return out


def calc_fid(real, gen, weights: str, feature: int = 2048, batch_size: int = 32):
    """``(fid, seconds in the metric's updates)``."""
    import torch
    from sonicdiffusionbayeslab_amd.metrics import FID
    metric = FID(feature=feature, weights=weights)
    seconds = 0.0
    for images, is_real in ((real, True), (gen, False)):
        groups = {}
        for img in images:
            groups.setdefault(tuple(img.shape), []).append(img)
        for items in groups.values():
            for s in range(0, len(items), batch_size):
                batch = torch.stack(items[s:s + batch_size])
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                metric.update(batch, real=is_real)
                torch.cuda.synchronize()
                seconds += time.perf_counter() - t0
    return float(metric.compute()), seconds


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description="Calculate FID between two image folders")
    ap.add_argument("real_dir", type=str, help="folder of real images")
    ap.add_argument("gen_dir", type=str, help="folder of generated images")
    ap.add_argument("--weights", type=str, required=True, help="local FID Inception-v3 state dict (.pth / .safetensors)")
    ap.add_argument("--feature", type=int, default=2048, choices=(64, 192, 768, 2048))
    ap.add_argument("--batch-size", type=int, default=32)
    args = ap.parse_args(argv)
    for d in (args.real_dir, args.gen_dir):
        if not os.path.isdir(d):
            raise ValueError(f"{d!r} is not a folder of images")
    real, gen = load_folder(args.real_dir), load_folder(args.gen_dir)
    if len(real) < 2 or len(gen) < 2:
        raise ValueError(f"FID needs at least two images per folder, found {len(real)} and {len(gen)}")
    fid, seconds = calc_fid(real, gen, args.weights, args.feature, args.batch_size)
    print(json.dumps({"fid": fid, "n_real": len(real), "n_gen": len(gen),
                      "images_per_s": (len(real) + len(gen)) / seconds if seconds > 0 else None,
                      "feature": args.feature, "weights": args.weights}), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
