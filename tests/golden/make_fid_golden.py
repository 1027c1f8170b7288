"""Regenerates tests/golden/fid_golden.npz and prints the figures the FID tests derive their gates from.

    python tests/golden/make_fid_golden.py

Everything is reference against reference, on the CPU: tests/inception_oracle.py in fp32 and in its bf16-emulating mode
(round_bf16=True), on the seeded weights and images of tests/fid_util.py.  No kernel of the library runs here.

  * e_tap: rel-L2 of the emulating run against the fp32 run, per tap, on the 4 images of the feature test (512 x 512);
  * e_fid: relative gap of the FID (24 real against 24 generated images, 96 x 80) between the two runs, features 64 and 2048;
  * the golden: the fp32 oracle's tap-64 and tap-2048 features of those 48 images, which the GPU metric test scores against
    (the oracle takes ~0.3 s per image on the host; the suite does not pay that for 48 images on every run).
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from sonicdiffusionbayeslab_amd.fid import frechet_distance  # noqa: E402
from tests.fid_util import METRIC_HW, metric_images, random_state_dict, seeded_images  # noqa: E402
from tests.inception_oracle import TAPS, inception_features  # noqa: E402


def fid_of(fr, fg):
    fr, fg = fr.double(), fg.double()
    return float(frechet_distance(fr.mean(0), torch.cov(fr.t()), fg.mean(0), torch.cov(fg.t())))


def main():
    sd = random_state_dict(0)
    imgs = seeded_images(4, 512, 512, 0)
    a, b = inception_features(sd, imgs), inception_features(sd, imgs, round_bf16=True)
    for tap in TAPS:
        print(f"e_tap[{tap}] = {float((a[tap].double() - b[tap].double()).norm() / a[tap].double().norm()):.4e}")
    real, gen = metric_images()
    both = torch.cat([real, gen])
    f32 = {64: [], 2048: []}
    fbf = {64: [], 2048: []}
    for s in range(0, both.shape[0], 8):
        x, y = inception_features(sd, both[s:s + 8]), inception_features(sd, both[s:s + 8], round_bf16=True)
        for t in f32:
            f32[t].append(x[t])
            fbf[t].append(y[t])
    n = real.shape[0]
    out = {}
    for t in f32:
        p, q = torch.cat(f32[t]), torch.cat(fbf[t])
        fa, fb = fid_of(p[:n], p[n:]), fid_of(q[:n], q[n:])
        print(f"feature {t}: fid fp32 {fa:.8g}, emulating {fb:.8g}, e_fid = {abs(fa - fb) / fa:.4e}")
        out[f"f{t}"] = p.numpy().astype(np.float32)
    out["hw"] = np.asarray(METRIC_HW)
    np.savez_compressed(os.path.join(ROOT, "tests", "golden", "fid_golden.npz"), **out)


if __name__ == "__main__":
    main()
