"""Measurements for profiles/taesd_notes.md: the tiny autoencoder (AutoencoderTiny / TAESD) against the AutoencoderKL.

    python tools/taesd_profile.py --part a [--out FILE]     decode / encode time per image, tiny and AutoencoderKL
    python tools/taesd_profile.py --part b                  conv64_kernel per decoder level against sd_op_conv3x3, rooflines
    python tools/taesd_profile.py --part c                  prompt strings to pictures: LCM-4 at batch 32, DDIM-50 at batch 8
    python tools/taesd_profile.py --part trace              one decode and one encode, for `rocprofv3 --kernel-trace --stats -- ...`

Device events around every timed call, a warm-up of every shape, old and new ALTERNATED inside one repeat loop (other work
shares the host: a difference is read against the spread of the repeats), FLOP and bytes computed from the shapes here.
One JSON line per figure, to stdout and (``--out``) appended to a file.  No GPU: the script fails (nothing is estimated)."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from sonicdiffusionbayeslab_amd import _lib  # noqa: E402

PEAK_BF16_FLOPS = 2.5e15        # dense bf16 MFMA (MI355X data sheet)
PEAK_HBM_BPS = 6.3e12           # achievable HBM3E bandwidth (measured float4 copy)
OUT = None


def emit(rec):
    line = json.dumps(rec)
    print(line, flush=True)
    if OUT:
        with open(OUT, "a") as f:
            f.write(line + "\n")


def timed(fn, reps):
    """Milliseconds per call of ``fn`` by device events, one figure per repeat."""
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return out


def alternate(fns, reps, warmup=2):
    """{name: [ms per repeat]} with the callables run in turn inside every repeat."""
    for _ in range(warmup):
        for f in fns.values():
            f()
    torch.cuda.synchronize()
    res = {k: [] for k in fns}
    for _ in range(reps):
        for k, f in fns.items():
            res[k] += timed(f, 1)
    return res


def stats(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4), "n": len(ms)}


def tiny_flops(lh, lw, half):
    """FLOP of one image through a half, from the layer table's shapes (2 x multiply-adds)."""
    from sonicdiffusionbayeslab_amd.vae import TINY_DECODER_LAYERS, TINY_ENCODER_LAYERS
    h, w = (lh, lw) if half == "decoder" else (8 * lh, 8 * lw)
    total = 0
    for kind, _ in (TINY_DECODER_LAYERS if half == "decoder" else TINY_ENCODER_LAYERS):
        if kind == "up":
            h, w = 2 * h, 2 * w
        elif kind == "down":
            h, w = h // 2, w // 2
        cin = {"entry": 4 if half == "decoder" else 3}.get(kind, 64)
        cout = {"exit": 3 if half == "decoder" else 4}.get(kind, 64)
        total += (3 if kind == "block" else 1) * 2 * 9 * cin * cout * h * w
    return total


def part_a(args):
    from sonicdiffusionbayeslab_amd.vae import (HipTinyVaeDecoder, HipTinyVaeEncoder, HipVaeDecoder, HipVaeEncoder, VaeConfig,
                                                make_synthetic_tiny_vae_state_dict, make_synthetic_vae_state_dict)
    tsd = make_synthetic_tiny_vae_state_dict()
    tdec, tenc = HipTinyVaeDecoder(tsd), HipTinyVaeEncoder(tsd)
    kcfg = VaeConfig()
    ksd = make_synthetic_vae_state_dict(kcfg)
    kdec, kenc = HipVaeDecoder(kcfg, ksd), HipVaeEncoder(kcfg, ksd)
    B = args.batch
    for side in (64, 96):
        g = torch.Generator().manual_seed(side)
        z = torch.randn((B, 4, side, side), generator=g).cuda()
        img = torch.rand((B, 3, 8 * side, 8 * side), generator=g).cuda()
        res = alternate({"tiny_decode": lambda: tdec.decode(z, unit_range=True, chunk=B),
                         "kl_decode": lambda: kdec.decode(z, 1.0 / 0.18215, chunk=B),
                         "tiny_encode": lambda: tenc.encode(img, chunk=B),
                         "kl_encode": lambda: kenc.encode(img, chunk=B)}, args.reps)
        for k, ms in res.items():
            rec = {"part": "a", "what": k, "image": 8 * side, "batch": B, **stats(ms),
                   "ms_per_image": round(statistics.median(ms) / B, 4)}
            if k.startswith("tiny"):
                fl = tiny_flops(side, side, "decoder" if "decode" in k else "encoder") * B
                rec["gflop_per_image"] = round(fl / B / 1e9, 2)
                rec["achieved_tflops"] = round(fl / (statistics.median(ms) * 1e-3) / 1e12, 1)
            emit(rec)


def part_b(args):
    lib = _lib.load()
    B = args.batch
    g = torch.Generator().manual_seed(1)
    w = (torch.randn(64, 64, 3, 3, generator=g) / 24.0).to(torch.bfloat16).float()
    packed = torch.empty(9 * 64 * 64, dtype=torch.int16)
    lib.sd_op_conv64_pack(w.contiguous().data_ptr(), packed.data_ptr())
    wp = packed.cuda()
    w3 = w.permute(0, 2, 3, 1).reshape(64, 9, 1, 64).permute(0, 2, 1, 3).contiguous().to(torch.bfloat16).cuda()     # [O][I/64][9][64]
    bias = torch.zeros(64).cuda()
    st = torch.cuda.current_stream().cuda_stream
    for side in (64, 128, 256, 512):
        x = torch.randn((B, side, side, 64), generator=g).to(torch.bfloat16).cuda()
        y1, y2 = torch.empty_like(x), torch.empty_like(x)

        def new():
            _lib.check(lib.sd_op_conv64(st, x.data_ptr(), wp.data_ptr(), bias.data_ptr(), None, y1.data_ptr(), B, side, side, 0, 1))

        def old():
            _lib.check(lib.sd_op_conv3x3(st, x.data_ptr(), w3.data_ptr(), bias.data_ptr(), None, None, y2.data_ptr(), B, side, side,
                                         64, 64, 1, 0))

        fns = {"conv64": new}
        try:
            old()
            torch.cuda.synchronize()
            fns["conv3x3"] = old
        except _lib.SdHipError as e:
            emit({"part": "b", "side": side, "conv3x3": f"refused: {e}"})
        res = alternate(fns, args.reps)
        flop = 2.0 * 9 * 64 * 64 * B * side * side
        byts = 2.0 * B * side * side * 128 + 9 * 64 * 64 * 2            # input once + output once + the weights
        floor_s = max(flop / PEAK_BF16_FLOPS, byts / PEAK_HBM_BPS)
        for k, ms in res.items():
            t = statistics.median(ms) * 1e-3
            emit({"part": "b", "kernel": k, "side": side, "batch": B, **stats(ms), "tflops": round(flop / t / 1e12, 1),
                  "tbytes_per_s": round(byts / t / 1e12, 2), "flop_per_byte": round(flop / byts, 1),
                  "bound": "mfma" if flop / PEAK_BF16_FLOPS > byts / PEAK_HBM_BPS else "hbm",
                  "share_of_floor": round(floor_s / t, 3)})
        if "conv3x3" in res:       # ReLU only in the new kernel: compare the pre-activation signs away
            d = (y1.float() - y2.float().clamp(min=0)).abs().max().item()
            emit({"part": "b", "side": side, "max_abs_diff_conv64_vs_relu_conv3x3": d})


def part_c(args):
    from sonicdiffusionbayeslab_amd.models import StableDiffusionModel
    from sonicdiffusionbayeslab_amd.registry import schedulers_registry
    from sonicdiffusionbayeslab_amd.schedulers import PNDMConfigStub
    model = StableDiffusionModel().to("cuda:0")
    prompts = [f"a photograph of an astronaut riding a horse, number {i}" for i in range(32)]
    keep = None

    def run(n_prompts, steps, gs, x0):
        out, secs, prev = model(prompts[:n_prompts], num_inference_steps=steps, guidance_scale=gs, output_type="pt",
                                generator=torch.Generator().manual_seed(29), collect_x0=x0)
        torch.cuda.synchronize()
        return secs

    for name, sched, n_prompts, steps, gs, x0 in (("lcm4_b32", "lcm_scheduler", 32, 4, 0.0, False),
                                                  ("ddim50_b8_x0", "ddim_scheduler", 8, 50, 7.5, True)):
        model.scheduler = schedulers_registry[sched].from_config(PNDMConfigStub().config)
        res = {"none": [], "previews": [], "all": []}
        loop = {"none": [], "previews": [], "all": []}
        for rep in range(args.reps_e2e + 1):                 # repeat 0 warms every variant up
            for use in ("none", "previews", "all"):
                if use != "none":
                    model.load_tiny_vae("madebyollin/taesd", use_for=use)
                    if keep:             # the same name = the same weights: no handle is built inside a timed call
                        model.tiny_vae_decoder, model.tiny_vae_encoder = keep
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                secs = run(n_prompts, steps, gs, x0)
                b.record()
                b.synchronize()
                if use != "none":
                    keep = (model.tiny_vae_decoder, model.tiny_vae_encoder)
                    model.unload_tiny_vae()
                if rep:
                    res[use].append(a.elapsed_time(b))
                    loop[use].append(secs * 1e3)
        for use in res:
            emit({"part": "c", "what": name, "tiny_vae": use, "images": n_prompts, **stats(res[use]),
                  "sampling_loop_median_ms": round(statistics.median(loop[use]), 2),
                  "images_per_s": round(n_prompts / (statistics.median(res[use]) * 1e-3), 1)})


def part_trace(args):
    from sonicdiffusionbayeslab_amd.vae import HipTinyVaeDecoder, HipTinyVaeEncoder, make_synthetic_tiny_vae_state_dict
    tsd = make_synthetic_tiny_vae_state_dict()
    tdec, tenc = HipTinyVaeDecoder(tsd), HipTinyVaeEncoder(tsd)
    z = torch.randn((args.batch, 4, 64, 64)).cuda()
    img = torch.rand((args.batch, 3, 512, 512)).cuda()
    for _ in range(3):
        tdec.decode(z, unit_range=True, chunk=args.batch)
        tenc.encode(img, chunk=args.batch)
    torch.cuda.synchronize()
    emit({"part": "trace", "decodes": 3, "encodes": 3, "batch": args.batch, "image": 512})


def main():
    global OUT
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=["a", "b", "c", "trace"], required=True)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--reps-e2e", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    OUT = args.out
    if not torch.cuda.is_available():
        raise SystemExit("tools/taesd_profile.py needs an MI355X: nothing is estimated without one")
    torch.cuda.set_device(0)
    {"a": part_a, "b": part_b, "c": part_c, "trace": part_trace}[args.part](args)


if __name__ == "__main__":
    main()
