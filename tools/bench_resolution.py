"""Throughput of the sampling loop at several image sizes (height / width per call): 50-step DDIM with CFG at batch 8 on
seeded synthetic SD-1.5 weights, timed as bench.py times its flagship run (best of --runs after one warm-up run).
Then, per UNet level, the resnet 3x3 conv (UNet batch 16: batch 8 with CFG) timed on the kernel the selection rule picks
and on the implicit-GEMM kernel (SD_CONV_HALO_GEN=0), through sd_op_conv3x3.

    python tools/bench_resolution.py [--sizes 512x512,512x768,768x512,768x768] [--runs 2] [--out FILE]

Prints one JSON line per size and one per (size, level)."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402


def conv_ms(lib, B, H, W, C, iters=20):
    """Mean time of one sd_op_conv3x3 (stride 1, C -> C channels, bias + residual as in a resnet conv2)."""
    from sonicdiffusionbayeslab_amd import _lib
    x = torch.randn(B, H, W, C, device="cuda").to(torch.bfloat16)
    w = (torch.randn(C, C // 64, 9, 64, device="cuda") / (3 * C ** 0.5)).to(torch.bfloat16)
    b = torch.randn(C, device="cuda")
    r = torch.randn(B, H, W, C, device="cuda").to(torch.bfloat16)
    y = torch.empty(B, H, W, C, device="cuda", dtype=torch.bfloat16)
    st = torch.cuda.current_stream().cuda_stream
    run = lambda: _lib.check(lib.sd_op_conv3x3(st, x.data_ptr(), w.data_ptr(), b.data_ptr(), None, r.data_ptr(), y.data_ptr(),
                                               B, H, W, C, C, 1, 0))
    run()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(iters):
        run()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def level_convs(lib, size, batch, out):
    height, width = (int(v) for v in size.lower().split("x"))
    for lev, C in enumerate((320, 640, 1280, 1280)):
        H, W = (height // 8) >> lev, (width // 8) >> lev
        B = 2 * batch
        kern = lib.sd_op_conv3x3_kernel(B * H * W, C, C, H, W, 1, 0, 0)
        picked = conv_ms(lib, B, H, W, C)
        os.environ["SD_CONV_HALO_GEN"] = "0"
        try:
            gemm = conv_ms(lib, B, H, W, C)
            kern_off = lib.sd_op_conv3x3_kernel(B * H * W, C, C, H, W, 1, 0, 0)
        finally:
            del os.environ["SD_CONV_HALO_GEN"]
        rec = dict(size=size, level=lev, conv=f"{B}x{H}x{W}x{C}", kernel=kern, ms=round(picked, 4),
                   kernel_without_geometry_mode=kern_off, ms_without_geometry_mode=round(gemm, 4),
                   speedup=round(gemm / picked, 3))
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            with open(out, "a") as f:
                f.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="512x512,512x768,768x512,768x768")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--runs", type=int, default=2, help="timed sampling runs per size (after one warm-up run)")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()

    from sonicdiffusionbayeslab_amd.models import StableDiffusionModel
    from sonicdiffusionbayeslab_amd.registry import schedulers_registry
    from sonicdiffusionbayeslab_amd.weights import UNetConfig, make_synthetic_state_dict

    torch.cuda.set_device(0)
    cfg = UNetConfig(sample_size=64)
    model = StableDiffusionModel(unet_config=cfg, state_dict=make_synthetic_state_dict(cfg, seed=1234)).to("cuda:0")
    model.scheduler = schedulers_registry["ddim_scheduler"].from_config(model.scheduler.config)
    g = torch.Generator().manual_seed(7)
    pe = torch.randn((args.batch, 77, 768), generator=g)
    ne = torch.randn((args.batch, 77, 768), generator=g)
    for size in args.sizes.split(","):
        height, width = (int(v) for v in size.lower().split("x"))
        lat = torch.randn((args.batch, 4, height // 8, width // 8), generator=g)
        run = lambda: model(prompt_embeds=pe, negative_prompt_embeds=ne, latents=lat, num_inference_steps=args.steps,
                            guidance_scale=7.5, output_type="latent", height=height, width=width, collect_x0=False)
        run()
        secs = []
        for _ in range(args.runs):
            _, s, _ = run()
            secs.append(s)
        loop = min(secs)
        rec = dict(size=size, batch=args.batch, steps=args.steps, loop_s=round(loop, 4),
                   images_per_s=round(args.batch / loop, 3),
                   megapixels_per_s=round(args.batch * height * width / 1e6 / loop, 3))
        line = json.dumps(rec)
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")
    from sonicdiffusionbayeslab_amd import _lib
    lib = _lib.load()
    for size in args.sizes.split(","):
        level_convs(lib, size, args.batch, args.out)


if __name__ == "__main__":
    main()
