"""Time per image pair of ImageReward scoring on libsdhip at the v1.0 shape (ViT-L/16 + BERT-base with 12 cross-attending
layers, synthetic weights), on seeded uint8 images already on the GPU.  A pair is what the win-rate metric scores per prompt:
the dataset's real image and the generated one, i.e. two ``score`` calls per batch of pairs.  Prints one JSON line.

    timeout -k 10 600 python tools/image_reward_speed.py [--batches 8 32] [--size 512] [--iters 5] [--skip-torch]
    rocprofv3 --kernel-trace --output-format csv -d OUT -- python tools/image_reward_speed.py --once 8
    python tools/image_reward_speed.py --count-launches OUT

``--once B``: build the model and run exactly ONE ``score`` call of batch B (nothing else launches a kernel), for a kernel
trace in a run of its own; ``--count-launches DIR`` then counts the rows of the trace's ``*kernel_trace.csv``.

For orientation only, beside the HIP numbers: the fp32 PyTorch restatement of the model (tests/image_reward_oracle.py, the
only other implementation there is offline) run on the same GPU with the same weights, on pixel values preprocessed once
on the host (its Pillow preprocessing is not timed)."""
from __future__ import annotations

import argparse
import csv
import glob
import json
import os
import re
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WORDS = ["a", "photo", "of", "the", "cat", "on", "red", "tree", "bird", "blue", "house", "water", "sky"]


def count_launches(d: str) -> int:
    files = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
    if len(files) != 1:
        raise SystemExit(f"expected one *kernel_trace.csv under {d}, found {files}")
    rows = list(csv.DictReader(open(files[0])))
    names = {}
    for r in rows:
        m = re.search(r"(\w+_kernel|__amd_\w+)", r.get("Kernel_Name", "?"))
        n = m.group(1) if m else r.get("Kernel_Name", "?")[:60]
        names[n] = names.get(n, 0) + 1
    print(json.dumps({"launches": len(rows), "by_kernel": dict(sorted(names.items(), key=lambda kv: -kv[1]))}))
    return 0


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[8, 32])
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--once", type=int, default=0)
    ap.add_argument("--count-launches", default=None)
    ap.add_argument("--skip-torch", action="store_true")
    a = ap.parse_args()
    if a.count_launches:
        return count_launches(a.count_launches)
    from sonicdiffusionbayeslab_amd import image_reward as IR
    from tests import image_reward_util as U
    vocab = U.synthetic_vocab()
    cfg = IR.ImageRewardConfig(vocab_size=len(vocab))
    sd = IR.make_synthetic_image_reward_state_dict(cfg, seed=1)
    tok = IR.BertWordPieceTokenizer({t: i for i, t in enumerate(vocab)}, max_length=cfg.max_text_len)
    m = IR.HipImageReward(cfg, sd, tok)
    g = torch.Generator().manual_seed(0)
    nmax = max(a.batches + [a.once])
    imgs = torch.randint(0, 256, (2 * nmax, 3, a.size, a.size), generator=g, dtype=torch.uint8).to("cuda")
    prompts = [" ".join(WORDS[(i * 7 + j * 3) % len(WORDS)] for j in range(4 + i % 9)) for i in range(nmax)]
    if a.once:
        m.score(prompts[:a.once], imgs[:a.once])
        torch.cuda.synchronize()
        return 0
    res = {"model": "ImageReward-v1.0 shape (synthetic weights)", "size": a.size, "iters": a.iters, "hip": {}, "torch_fp32_same_gpu": {}}
    for b in a.batches:
        real, gen = imgs[:b], imgs[nmax:nmax + b]
        m.score(prompts[:b], real)                  # plan, workspace, first launches
        torch.cuda.synchronize()
        ts = []
        for _ in range(a.iters):
            t0 = time.perf_counter()
            m.score(prompts[:b], real)
            m.score(prompts[:b], gen)
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        ts.sort()
        res["hip"][str(b)] = {"ms_per_pair_median": 1e3 * ts[len(ts) // 2] / b, "ms_per_pair_min": 1e3 * ts[0] / b,
                              "ms_per_pair_max": 1e3 * ts[-1] / b}
    if not a.skip_torch:
        from tests import image_reward_oracle as O
        dsd = {k: v.to("cuda") for k, v in sd.items()}
        for b in a.batches:
            pix = [O.preprocess(list(imgs[s:s + b].cpu()), cfg).to("cuda") for s in (0, nmax)]
            ids, mask = (t.to("cuda") for t in tok(prompts[:b]))

            def run(p):
                tokens = O.vision_forward(dsd, cfg, p)
                return O.reward_head(dsd, cfg, O.text_forward(dsd, cfg, ids, mask, tokens)[:, 0])

            run(pix[0])
            torch.cuda.synchronize()
            ts = []
            for _ in range(a.iters):
                t0 = time.perf_counter()
                run(pix[0]); run(pix[1])
                torch.cuda.synchronize()
                ts.append(time.perf_counter() - t0)
            ts.sort()
            res["torch_fp32_same_gpu"][str(b)] = {"ms_per_pair_median": 1e3 * ts[len(ts) // 2] / b, "ms_per_pair_min": 1e3 * ts[0] / b,
                                                  "ms_per_pair_max": 1e3 * ts[-1] / b}
    print(json.dumps(res), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
