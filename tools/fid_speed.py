"""Images/s of the FID feature extractor on libsdhip (preprocessing + Inception-v3 up to the tap + global mean), on seeded
uint8 images with synthetic weights of the checkpoint's shapes.  Prints one JSON line per tap: images/s with the images
already on the device, with the host -> device copy, and with the fp64 statistics update (sd_fid_accumulate) as the metric
runs it.  There is no host path to compare with: torchmetrics / torch-fidelity / torchvision do not exist offline.

    timeout -k 10 600 python tools/fid_speed.py [--images 64] [--size 512] [--batch 32] [--taps 2048,64] [--loops 3]

For a per-kernel breakdown run the same command under ``rocprofv3 --kernel-trace --stats -d <dir> --``."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--taps", type=str, default="2048,64")
    ap.add_argument("--loops", type=int, default=3)
    a = ap.parse_args()
    from sonicdiffusionbayeslab_amd.fid import HipInceptionFeatures, fid_accumulate, make_synthetic_inception_state_dict
    net = HipInceptionFeatures.from_state_dict(make_synthetic_inception_state_dict(1))
    g = torch.Generator().manual_seed(0)
    imgs = torch.randint(0, 256, (a.images, 3, a.size, a.size), generator=g, dtype=torch.uint8)
    dev = imgs.to("cuda")
    for tap in (int(t) for t in a.taps.split(",")):
        res = {"tap": tap, "images": a.images, "size": a.size, "batch": a.batch, "loops": a.loops,
               "model": "FID Inception-v3 (synthetic weights)"}
        net.features(dev[:a.batch], tap)          # workspace, first launches
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.loops):
            for s in range(0, a.images, a.batch):
                net.features(dev[s:s + a.batch], tap)
        torch.cuda.synchronize()
        res["images_per_s"] = a.loops * a.images / (time.perf_counter() - t0)
        total = torch.zeros(tap, dtype=torch.float64, device="cuda")
        cov = torch.zeros(tap, tap, dtype=torch.float64, device="cuda")
        count = torch.zeros(1, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.loops):
            for s in range(0, a.images, a.batch):
                fid_accumulate(net.features(imgs[s:s + a.batch], tap), total, cov, count)
        torch.cuda.synchronize()
        res["images_per_s_incl_upload_and_statistics"] = a.loops * a.images / (time.perf_counter() - t0)
        assert int(count.item()) == a.loops * a.images
        print(json.dumps(res), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
