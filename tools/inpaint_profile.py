"""Loop seconds and launch counts of inpainting beside text-to-image (profiles/inpaint_notes.md).

    python tools/inpaint_profile.py --mode both                          # loop seconds, profiler off, runs alternated
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT/t2i     -- python tools/inpaint_profile.py --mode t2i --runs 1 --warmup 0
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT/inpaint -- python tools/inpaint_profile.py --mode inpaint --runs 1 --warmup 0
    python tools/inpaint_profile.py --summarise OUT/t2i OUT/inpaint      # launches per kernel, side by side

Synthetic SD-1.5-shaped weights, seeded inputs, DDIM, CFG 7.5; the mask is a centred box over half of each side.  The loop
seconds are the pipeline's own (device-synchronised wall clock of the denoising loop; encoding and mask processing sit
outside, like text encoding).  ``--in-channels 9`` runs the inpainting loop on a 9-channel UNet (no text-to-image leg).
"""
import argparse
import csv
import glob
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def summarise(dirs):
    tables = []
    for d in dirs:
        files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        if len(files) != 1:
            raise SystemExit(f"{d}: expected one *kernel_stats.csv, found {files}")
        with open(files[0]) as f:
            tables.append({r["Name"]: (int(r["Calls"]), float(r["TotalDurationNs"])) for r in csv.DictReader(f)})
    names = sorted(set().union(*tables), key=lambda n: -max(t.get(n, (0, 0))[1] for t in tables))
    print("| kernel | " + " | ".join(f"launches {os.path.basename(os.path.normpath(d))} | ms" for d in dirs) + " |")
    print("|---|" + "---|---|" * len(dirs))
    for n in names:
        row = [f"{t.get(n, (0, 0))[0]} | {t.get(n, (0, 0.0))[1] / 1e6:.3f}" for t in tables]
        short = n.replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0][:70]
        print(f"| `{short}` | " + " | ".join(row) + " |")
    print("| total | " + " | ".join(f"{sum(c for c, _ in t.values())} | {sum(ns for _, ns in t.values()) / 1e6:.3f}" for t in tables) + " |")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["t2i", "inpaint", "both"], default="both")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--ddim-steps", type=int, default=50)
    ap.add_argument("--sample-size", type=int, default=64)
    ap.add_argument("--strength", type=float, default=1.0)
    ap.add_argument("--in-channels", type=int, default=4, choices=[4, 9])
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--summarise", nargs="+", metavar="DIR")
    args = ap.parse_args()
    if args.summarise:
        return summarise(args.summarise)

    import torch
    from sonicdiffusionbayeslab_amd.models import StableDiffusionModel
    from sonicdiffusionbayeslab_amd.registry import schedulers_registry
    from sonicdiffusionbayeslab_amd.weights import UNetConfig, make_synthetic_state_dict
    if not torch.cuda.is_available():
        raise SystemExit("inpaint_profile needs an MI355X: no GPU, no number")
    if args.in_channels == 9 and args.mode != "inpaint":
        raise SystemExit("--in-channels 9 runs --mode inpaint only")
    cfg = UNetConfig(sample_size=args.sample_size, in_channels=args.in_channels)
    model = StableDiffusionModel(unet_config=cfg, state_dict=make_synthetic_state_dict(cfg, seed=1234)).to("cuda:0")
    model.scheduler = schedulers_registry["ddim_scheduler"].from_config(model.scheduler.config)
    B, S = args.batch, args.sample_size * 8
    g = torch.Generator().manual_seed(29)
    pe, ne = torch.randn(B, 77, 768, generator=g), torch.randn(B, 77, 768, generator=g)
    lat = torch.randn(B, 4, args.sample_size, args.sample_size, generator=g)
    img = torch.rand(B, 3, S, S, generator=g).cuda()
    mask = torch.zeros(B, 1, S, S)
    mask[:, :, S // 4:3 * S // 4, S // 4:3 * S // 4] = 1.0
    common = dict(prompt_embeds=pe, negative_prompt_embeds=ne, num_inference_steps=args.ddim_steps, guidance_scale=7.5,
                  output_type="latent", collect_x0=False)
    calls = {"t2i": lambda: model(latents=lat, **common),
             "inpaint": lambda: model(image=img, mask_image=mask.cuda(), strength=args.strength,
                                      generator=torch.Generator().manual_seed(3), **common)}
    modes = ["t2i", "inpaint"] if args.mode == "both" else [args.mode]
    secs = {m: [] for m in modes}
    for i in range(args.warmup + args.runs):
        for m in modes:                                  # alternated: both legs see the same drift of the box
            _, s, _ = calls[m]()
            if i >= args.warmup:
                secs[m].append(s)
    res = {"batch": B, "ddim_steps": args.ddim_steps, "pixels": S, "strength": args.strength, "in_channels": args.in_channels,
           "steps_run": model.num_timesteps, "runs": args.runs, "warmup": args.warmup,
           "loop_seconds": {m: {"min": min(v), "median": sorted(v)[len(v) // 2], "all": v} for m, v in secs.items()}}
    if len(modes) == 2:
        res["inpaint_over_t2i_median"] = res["loop_seconds"]["inpaint"]["median"] / res["loop_seconds"]["t2i"]["median"]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
