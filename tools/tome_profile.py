"""What Token Merging nets (profiles/tome_notes.md): per-forward time and the per-op time of the four tome kernels at several
image sizes and merge ratios, and the 50-step DDIM loop in images/s.

    python tools/tome_profile.py --size 64 --batch 8                       # 512 px, UNet batch 16
    python tools/tome_profile.py --size 96 --batch 4 --loop-ratios 0 0.5   # 768 px
    python tools/tome_profile.py --size 128 --batch 2 --loop-ratios 0 0.5  # 1024 px

Synthetic SD-1.5-shaped weights, seeded inputs, DDIM, CFG 7.5.  The comparison is the SAME build's ratio-0 run (the plans of a
handle that never saw Token Merging).  Forward times are free-running (no per-launch events), the ratios alternated inside
every round so that all see the same drift of the box; the per-op figures come from one forward with an event per launch
(each reading carries ~4-5 us of launch latency that a free-running stream hides).  Loop seconds are the pipeline's own
(device-synchronised wall clock of the denoising loop, per-step choice upload included)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

OPS = ("tome_match", "tome_select", "tome_merge", "tome_unmerge", "attention", "gemm", "layernorm", "xattn_fused", "replicate")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=64, help="latent side (64 = 512 px)")
    ap.add_argument("--batch", type=int, default=8, help="latent batch (the UNet batch is twice that: CFG)")
    ap.add_argument("--ratios", type=float, nargs="+", default=[0.0, 0.25, 0.5, 0.75])
    ap.add_argument("--loop-ratios", type=float, nargs="*", default=None, help="ratios of the DDIM loop (default: --ratios)")
    ap.add_argument("--max-downsample", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--forwards", type=int, default=10)
    ap.add_argument("--ddim-steps", type=int, default=50)
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=1)
    args = ap.parse_args()

    import torch
    from sonicdiffusionbayeslab_amd.models import StableDiffusionModel
    from sonicdiffusionbayeslab_amd.registry import schedulers_registry
    from sonicdiffusionbayeslab_amd.weights import UNetConfig, make_synthetic_state_dict
    if not torch.cuda.is_available():
        raise SystemExit("tome_profile needs an MI355X: no GPU, no number")
    S, B = args.size, args.batch
    UB = 2 * B
    cfg = UNetConfig(sample_size=S)
    model = StableDiffusionModel(unet_config=cfg, state_dict=make_synthetic_state_dict(cfg, seed=1234)).to("cuda:0")
    model.scheduler = schedulers_registry["ddim_scheduler"].from_config(model.scheduler.config)
    g = torch.Generator().manual_seed(29)
    pe, ne = torch.randn(B, 77, 768, generator=g), torch.randn(B, 77, 768, generator=g)
    lat = torch.randn(B, 4, S, S, generator=g)
    net, ctx, x = model.unet, torch.cat([ne, pe]).cuda(), lat.cuda()
    net.set_deepcache(-1)

    def setup(ratio):
        net.set_tome(ratio, args.max_downsample)
        net.set_context(ctx)
        blocks = net.tome_blocks()
        if blocks:
            n = sum((b["h"] // 2) * (b["w"] // 2) for b in blocks)
            net.set_tome_choice(torch.randint(4, (n,), generator=torch.Generator().manual_seed(5), dtype=torch.uint8).cuda())
        return blocks

    res = {"latent": S, "pixels": 8 * S, "batch": B, "unet_batch": UB, "max_downsample": args.max_downsample, "ratios": {}}
    for ratio in args.ratios:          # one forward with an event per launch: launches and milliseconds per op kind
        blocks = setup(ratio)
        for _ in range(2):
            prof = net.forward_profiled(x, UB, 501.0)
        res["ratios"][str(ratio)] = {
            "merging_blocks": len(blocks), "merged_per_block": [b["r"] for b in blocks],
            "launches": sum(v["launches"] for v in prof.values()),
            "per_launch_event_ms_total": sum(v["ms"] for v in prof.values()),
            "op_ms": {k: prof[k]["ms"] for k in OPS if k in prof}, "op_launches": {k: prof[k]["launches"] for k in OPS if k in prof},
            "forward_ms": []}
    for _ in range(args.rounds):       # free-running forwards, the ratios alternated
        for ratio in args.ratios:
            setup(ratio)
            for _ in range(2):
                net.forward_latents(x, UB, 501.0)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(args.forwards):
                net.forward_latents(x, UB, 501.0)
            b.record()
            torch.cuda.synchronize()
            res["ratios"][str(ratio)]["forward_ms"].append(a.elapsed_time(b) / args.forwards)
    base = sorted(res["ratios"][str(args.ratios[0])]["forward_ms"])[args.rounds // 2]
    for r in res["ratios"].values():
        r["forward_ms_median"] = sorted(r["forward_ms"])[args.rounds // 2]
        r["forward_over_first_ratio"] = r["forward_ms_median"] / base
    net.set_tome(0.0)

    loop_ratios = args.ratios if args.loop_ratios is None else args.loop_ratios
    if loop_ratios and args.ddim_steps > 0:
        common = dict(prompt_embeds=pe, negative_prompt_embeds=ne, latents=lat, num_inference_steps=args.ddim_steps, guidance_scale=7.5,
                      output_type="latent", collect_x0=False, height=8 * S, width=8 * S)
        secs = {str(r): [] for r in loop_ratios}
        for i in range(args.warmup + args.runs):
            for r in loop_ratios:                           # alternated
                model.apply_tome(ratio=r, max_downsample=args.max_downsample)
                _, s, _ = model(**common)
                if i >= args.warmup:
                    secs[str(r)].append(s)
        model.remove_tome()
        res["ddim"] = {"steps": args.ddim_steps, "runs": args.runs, "warmup": args.warmup,
                       "loop_seconds": {k: {"min": min(v), "median": sorted(v)[len(v) // 2], "all": v} for k, v in secs.items()},
                       "images_per_s": {k: B / sorted(v)[len(v) // 2] for k, v in secs.items()}}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
