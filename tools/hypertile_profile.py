"""What HyperTile nets (profiles/hypertile_notes.md): per-forward time, the attention column and the time of the two new launches
at several image sizes and settings, and the 50-step DDIM loop in images/s.  One process per size.

    python tools/hypertile_profile.py --size 64 --batch 8 --settings off 32:0 32:1 16:0    # 512 px, UNet batch 16
    python tools/hypertile_profile.py --size 96 --batch 4 --ddim-steps 0                    # 768 px
    python tools/hypertile_profile.py --size 128 --batch 2                                  # 1024 px

A setting is ``off``, ``T:max_depth`` (T = the tile side in tokens = tile_size / 8: 32 = 256 px, 16 = 128 px) or ``tome:ratio``
(Token Merging at that ratio, max_downsample 1, for comparison in the same run).  Synthetic SD-1.5-shaped weights, seeded
inputs, DDIM, CFG 7.5.  The comparison is the SAME build's ``off`` run (the plans of a handle that never saw the setting).
Forward times are free-running (no per-launch events), the settings alternated inside every round so that all see the same drift
of the box; the per-op figures come from one forward with an event per launch (each reading carries ~4-5 us of launch latency
that a free-running stream hides).  Loop seconds are the pipeline's own (device-synchronised wall clock of the denoising loop)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

OPS = ("hypertile_gather", "hypertile_scatter", "attention", "gemm", "layernorm", "groupnorm", "xattn_fused", "replicate",
       "tome_match", "tome_select", "tome_merge", "tome_unmerge")


def parse_setting(s):
    """-> ("off",) | ("tile", T, max_depth) | ("tome", ratio)"""
    if s == "off":
        return ("off",)
    a, b = s.split(":")
    return ("tome", float(b)) if a == "tome" else ("tile", int(a), int(b))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=64, help="latent side (64 = 512 px)")
    ap.add_argument("--batch", type=int, default=8, help="latent batch (the UNet batch is twice that: CFG)")
    ap.add_argument("--settings", nargs="+", default=["off", "32:0", "32:1", "tome:0.5"])
    ap.add_argument("--loop-settings", nargs="*", default=None, help="settings of the DDIM loop (default: --settings)")
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
        raise SystemExit("hypertile_profile needs an MI355X: no GPU, no number")
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

    def setup(name):
        st = parse_setting(name)
        net.set_hypertile(0)
        net.set_tome(0.0)
        if st[0] == "tile":
            net.set_hypertile(st[1], st[2])
        elif st[0] == "tome":
            net.set_tome(st[1], 1)
        net.set_context(ctx)
        if st[0] == "tome":
            n = sum((b["h"] // 2) * (b["w"] // 2) for b in net.tome_blocks())
            net.set_tome_choice(torch.randint(4, (n,), generator=torch.Generator().manual_seed(5), dtype=torch.uint8).cuda())
        return net.hypertile_blocks()

    res = {"latent": S, "pixels": 8 * S, "batch": B, "unet_batch": UB, "settings": {}}
    for name in args.settings:         # one forward with an event per launch: launches and milliseconds per op kind
        blocks = setup(name)
        for _ in range(2):
            prof = net.forward_profiled(x, UB, 501.0)
        res["settings"][name] = {
            "tiled_blocks": [[b["rh"], b["rw"], b["nh"], b["nw"]] for b in blocks],
            "launches": sum(v["launches"] for v in prof.values()),
            "per_launch_event_ms_total": sum(v["ms"] for v in prof.values()),
            "op_ms": {k: prof[k]["ms"] for k in OPS if k in prof}, "op_launches": {k: prof[k]["launches"] for k in OPS if k in prof},
            "copy_bytes": sum(prof[k]["bytes"] for k in ("hypertile_gather", "hypertile_scatter") if k in prof),
            "forward_ms": []}
    for _ in range(args.rounds):       # free-running forwards, the settings alternated
        for name in args.settings:
            setup(name)
            for _ in range(2):
                net.forward_latents(x, UB, 501.0)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(args.forwards):
                net.forward_latents(x, UB, 501.0)
            b.record()
            torch.cuda.synchronize()
            res["settings"][name]["forward_ms"].append(a.elapsed_time(b) / args.forwards)
    base = sorted(res["settings"][args.settings[0]]["forward_ms"])[args.rounds // 2]
    for r in res["settings"].values():
        r["forward_ms_median"] = sorted(r["forward_ms"])[args.rounds // 2]
        r["forward_over_first_setting"] = r["forward_ms_median"] / base
    net.set_hypertile(0)
    net.set_tome(0.0)

    loop_settings = args.settings if args.loop_settings is None else args.loop_settings
    if loop_settings and args.ddim_steps > 0:
        common = dict(prompt_embeds=pe, negative_prompt_embeds=ne, latents=lat, num_inference_steps=args.ddim_steps, guidance_scale=7.5,
                      output_type="latent", collect_x0=False, height=8 * S, width=8 * S)
        secs = {name: [] for name in loop_settings}
        for i in range(args.warmup + args.runs):
            for name in loop_settings:                      # alternated
                st = parse_setting(name)
                model.disable_hypertile()
                model.remove_tome()
                if st[0] == "tile":
                    model.enable_hypertile(tile_size=8 * st[1], max_depth=st[2])
                elif st[0] == "tome":
                    model.apply_tome(ratio=st[1], max_downsample=1)
                _, s, _ = model(**common)
                if i >= args.warmup:
                    secs[name].append(s)
        model.disable_hypertile()
        model.remove_tome()
        res["ddim"] = {"steps": args.ddim_steps, "runs": args.runs, "warmup": args.warmup,
                       "loop_seconds": {k: {"min": min(v), "median": sorted(v)[len(v) // 2], "all": v} for k, v in secs.items()},
                       "images_per_s": {k: B / sorted(v)[len(v) // 2] for k, v in secs.items()}}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
