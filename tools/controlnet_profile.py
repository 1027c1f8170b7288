"""Cost of a ControlNet beside the plain loop (profiles/controlnet_notes.md).

    python tools/controlnet_profile.py                    # launches per kind with and without residuals, the time of the
                                                           # ControlNet forward, of the add launch and of the GroupNorms, DDIM loop
                                                           # seconds and images/s with / without a control image (alternated)
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT/<what> -- python tools/controlnet_profile.py --mode forward --what <what>
                                                           # <what> = controlnet | unet_control | unet_plain: N forwards of one kind
    python tools/controlnet_profile.py --summarise OUT/controlnet OUT/unet_control OUT/unet_plain --forwards N
                                                           # launches per forward and kernel time per forward, by kernel name

Synthetic SD-1.5-shaped weights and ControlNet (the seeded stand-in of a hub name), seeded inputs, DDIM, CFG 7.5, the same build
for both legs.  Loop seconds are the pipeline's own (device-synchronised wall clock of the denoising loop); the conditioning
embedding (``sd_controlnet_set_cond_hw``) sits outside it, like text encoding, and is timed on its own.
"""
import argparse
import csv
import glob
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def summarise(dirs, forwards):
    """Kernel statistics of the three traced runs: per kernel name the launches and microseconds PER FORWARD (calls // N; what is
    left over is the run's set-up -- set_context, the conditioning embedding -- and is reported apart)."""
    out = {}
    for d in dirs:
        files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        if not files:
            raise SystemExit(f"{d}: no *kernel_stats.csv")
        rows, setup_calls = [], 0
        with open(files[0]) as f:
            for r in csv.DictReader(f):
                calls, ns = int(r["Calls"]), float(r["TotalDurationNs"])
                per = calls // forwards
                setup_calls += calls - per * forwards
                if per:
                    rows.append({"kernel": r["Name"][:96], "launches_per_forward": per, "us_per_forward": ns / calls * per / 1e3})
        rows.sort(key=lambda r: -r["us_per_forward"])
        out[os.path.basename(os.path.normpath(d))] = {
            "launches_per_forward": sum(r["launches_per_forward"] for r in rows),
            "kernel_us_per_forward": sum(r["us_per_forward"] for r in rows), "setup_launches_in_the_run": setup_calls,
            "kernels": rows}
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["all", "forward"], default="all")
    ap.add_argument("--what", choices=["controlnet", "unet_control", "unet_plain"], default="controlnet")
    ap.add_argument("--forwards", type=int, default=10)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--ddim-steps", type=int, default=50)
    ap.add_argument("--sample-size", type=int, default=64)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--summarise", nargs="+", metavar="DIR")
    args = ap.parse_args()
    if args.summarise:
        return summarise(args.summarise, args.forwards)

    import torch
    from sonicdiffusionbayeslab_amd.models import StableDiffusionModel
    from sonicdiffusionbayeslab_amd.registry import schedulers_registry
    from sonicdiffusionbayeslab_amd.weights import UNetConfig, make_synthetic_state_dict
    if not torch.cuda.is_available():
        raise SystemExit("controlnet_profile needs an MI355X: no GPU, no number")
    S, B = args.sample_size, args.batch
    base = UNetConfig(sample_size=S)
    model = StableDiffusionModel(unet_config=base, state_dict=make_synthetic_state_dict(base, seed=1234))
    model.load_controlnet("lllyasviel/sd-controlnet-canny")      # a hub name: the seeded stand-in (weights_source says so)
    model.to("cuda:0")
    model.scheduler = schedulers_registry["ddim_scheduler"].from_config(model.scheduler.config)
    g = torch.Generator().manual_seed(29)
    pe, ne = torch.randn(B, 77, 768, generator=g), torch.randn(B, 77, 768, generator=g)
    lat = torch.randn(B, 4, S, S, generator=g)
    cond = torch.rand(B, 3, 8 * S, 8 * S, generator=g)
    model._size = (8 * S, 8 * S)
    net, cnet, ctx, x = model.unet, model._ensure_controlnet(), torch.cat([ne, pe]).cuda(), lat.cuda()
    UB = 2 * B

    net.set_deepcache(-1)
    net.set_context(ctx)
    cnet.set_context(ctx, S, S)
    cnet.set_cond(cond)
    torch.cuda.synchronize()
    t0 = time.time()
    cnet.set_cond(cond)
    torch.cuda.synchronize()
    set_cond_s = time.time() - t0
    buf = cnet.forward_residuals(x, UB, 501.0)

    def timed(fn, n):
        for _ in range(2):
            fn()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(n):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / n

    def control_forward():
        net.set_control_residuals(buf, 1.0, UB)
        net.forward_latents(x, UB, 501.0)

    def plain_forward():
        net.clear_control_residuals()
        net.forward_latents(x, UB, 501.0)

    if args.mode == "forward":
        fn = {"controlnet": lambda: cnet.forward_residuals(x, UB, 501.0), "unet_control": control_forward, "unet_plain": plain_forward}[args.what]
        for _ in range(args.forwards):
            fn()
        torch.cuda.synchronize()
        print(json.dumps({"what": args.what, "forwards": args.forwards, "unet_batch": UB, "latent": S}))
        return

    # one forward each way with an event per launch (each reading carries ~4-5 us): launches per kind, the add launch, the GroupNorms
    net.clear_control_residuals()
    for _ in range(2):
        prof_off = net.forward_profiled(x, UB, 501.0)
    net.set_control_residuals(buf, 1.0, UB)
    for _ in range(2):
        prof_on = net.forward_profiled(x, UB, 501.0)
    net.clear_control_residuals()
    res = {"batch": B, "unet_batch": UB, "latent": S,
           "launches_plain": {k: v["launches"] for k, v in prof_off.items() if v["launches"]},
           "launches_with_residuals": {k: v["launches"] for k, v in prof_on.items() if v["launches"]},
           "per_launch_event_ms_plain": sum(v["ms"] for v in prof_off.values()),
           "per_launch_event_ms_with_residuals": sum(v["ms"] for v in prof_on.values()),
           "residual_add_ms": prof_on["residual_add"]["ms"], "residual_add_algorithmic_MB": prof_on["residual_add"]["bytes"] / 1e6,
           "groupnorm_ms_plain": prof_off["groupnorm"]["ms"], "groupnorm_ms_with_residuals": prof_on["groupnorm"]["ms"],
           "conv3x3_ms_plain": prof_off["conv3x3"]["ms"], "conv3x3_ms_with_residuals": prof_on["conv3x3"]["ms"],
           "set_cond_seconds": set_cond_s}
    # free-running forwards (no per-launch events), alternated
    fw = {"controlnet_forward_ms": [], "unet_plain_forward_ms": [], "unet_with_residuals_forward_ms": []}
    for _ in range(3):
        fw["controlnet_forward_ms"].append(timed(lambda: cnet.forward_residuals(x, UB, 501.0), 10))
        fw["unet_plain_forward_ms"].append(timed(plain_forward, 10))
        fw["unet_with_residuals_forward_ms"].append(timed(control_forward, 10))
    net.clear_control_residuals()
    res.update({k: {"median": sorted(v)[1], "all": v} for k, v in fw.items()})
    common = dict(prompt_embeds=pe, negative_prompt_embeds=ne, latents=lat, num_inference_steps=args.ddim_steps, guidance_scale=7.5,
                  output_type="latent", collect_x0=False)
    calls = {"plain": lambda: model(**common), "control_image": lambda: model(control_image=cond, **common)}
    secs = {m: [] for m in calls}
    for i in range(args.warmup + args.runs):
        for m in calls:                                  # alternated: both legs see the same drift of the box
            _, s, _ = calls[m]()
            if i >= args.warmup:
                secs[m].append(s)
    res.update(ddim_steps=args.ddim_steps, runs=args.runs, warmup=args.warmup,
               loop_seconds={m: {"min": min(v), "median": sorted(v)[len(v) // 2], "all": v} for m, v in secs.items()},
               images_per_s={m: B / sorted(v)[len(v) // 2] for m, v in secs.items()})
    res["control_image_over_plain_median"] = res["loop_seconds"]["control_image"]["median"] / res["loop_seconds"]["plain"]["median"]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
