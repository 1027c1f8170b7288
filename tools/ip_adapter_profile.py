"""Cost of an IP-Adapter image prompt beside the plain loop (profiles/ip_adapter_notes.md).

    python tools/ip_adapter_profile.py                                   # launch counts per kind, the image branch's time per
                                                                          # forward, DDIM loop seconds with / without (alternated)
    rocprofv3 --pmc FETCH_SIZE --output-format csv -d OUT/rd -- python tools/ip_adapter_profile.py --mode forward
    rocprofv3 --pmc WRITE_SIZE --output-format csv -d OUT/wr -- python tools/ip_adapter_profile.py --mode forward
    python tools/ip_adapter_profile.py --summarise OUT/rd OUT/wr         # HBM bytes of the largest ip_xattn launches (counters only)

Synthetic SD-1.5-shaped weights and adapter, seeded inputs, DDIM, CFG 7.5, the same build for both legs.  Loop seconds are
the pipeline's own (device-synchronised wall clock of the denoising loop); the fold of the image prompt
(``sd_unet_set_ip_adapter_hw``) sits outside, like text encoding, and is timed on its own.
"""
import argparse
import csv
import glob
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def summarise(dirs):
    """FETCH_SIZE and WRITE_SIZE do not fit one pass on gfx950 (TCC slots): one counters-only run each, summarised together."""
    per = {}
    for d in dirs:
        files = glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True)
        if not files:
            raise SystemExit(f"{d}: no *counter_collection.csv")
        for fn in files:
            with open(fn) as f:
                for r in csv.DictReader(f):
                    if "ip_xattn" not in r["Kernel_Name"]:
                        continue
                    grid = int(r["Grid_Size"])
                    per.setdefault(grid, {}).setdefault(r["Counter_Name"], []).append(float(r["Counter_Value"]))
    if not per:
        raise SystemExit("no ip_xattn dispatch in the counters")
    grid = max(per)
    # FETCH_SIZE / WRITE_SIZE count kilobytes; on gfx950 FETCH_SIZE tallies a wide coalesced read stream at half its bytes
    out = {"largest_grid_threads": grid}
    for name, vals in per[grid].items():
        out[name + "_MB_per_launch_median"] = sorted(vals)[len(vals) // 2] / 1024.0
        out[name + "_launches"] = len(vals)
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["all", "forward"], default="all")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--ddim-steps", type=int, default=50)
    ap.add_argument("--sample-size", type=int, default=64)
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
        raise SystemExit("ip_adapter_profile needs an MI355X: no GPU, no number")
    E = StableDiffusionModel.IP_ADAPTER_EMBED_DIM
    base = UNetConfig(sample_size=args.sample_size)
    model = StableDiffusionModel(unet_config=base, state_dict=make_synthetic_state_dict(base, seed=1234))
    # a hub name: the seeded synthetic adapter of the published shape stands in (weights_source says so)
    model.load_ip_adapter("h94/IP-Adapter", subfolder="models", weight_name="ip-adapter_sd15.bin")
    model.to("cuda:0")
    model.scheduler = schedulers_registry["ddim_scheduler"].from_config(model.scheduler.config)
    B = args.batch
    g = torch.Generator().manual_seed(29)
    pe, ne = torch.randn(B, 77, 768, generator=g), torch.randn(B, 77, 768, generator=g)
    lat = torch.randn(B, 4, args.sample_size, args.sample_size, generator=g)
    emb = torch.randn(B, E, generator=g)
    net, ctx = model.unet, torch.cat([ne, pe]).cuda()
    full = torch.cat([torch.zeros_like(emb), emb]).cuda()

    # one forward each way: launches per kind and the new kind's time (hipEvent per launch: each reading carries ~4-5 us)
    net.set_deepcache(-1)
    net.set_context(ctx)
    net.clear_ip_adapter()
    for _ in range(2):
        prof_off = net.forward_profiled(lat.cuda(), 2 * B, 501.0)
    torch.cuda.synchronize()
    t0 = time.time()
    net.set_ip_adapter(full, 1.0)
    torch.cuda.synchronize()
    fold_s = time.time() - t0
    for _ in range(2):
        prof_on = net.forward_profiled(lat.cuda(), 2 * B, 501.0)
    res = {"batch": B, "unet_batch": 2 * B, "latent": args.sample_size,
           "launches_off": {k: v["launches"] for k, v in prof_off.items() if v["launches"]},
           "launches_on": {k: v["launches"] for k, v in prof_on.items() if v["launches"]},
           "forward_ms_off": sum(v["ms"] for v in prof_off.values()), "forward_ms_on": sum(v["ms"] for v in prof_on.values()),
           "ip_xattn_ms_per_forward": prof_on["ip_xattn"]["ms"], "ip_xattn_algorithmic_MB": prof_on["ip_xattn"]["bytes"] / 1e6,
           "set_ip_adapter_seconds_first_call": fold_s}
    if args.mode == "forward":
        net.forward_latents(lat.cuda(), 2 * B, 501.0)
        torch.cuda.synchronize()
        print(json.dumps(res))
        return
    common = dict(prompt_embeds=pe, negative_prompt_embeds=ne, latents=lat, num_inference_steps=args.ddim_steps, guidance_scale=7.5,
                  output_type="latent", collect_x0=False)
    calls = {"plain": lambda: model(**common), "image_prompt": lambda: model(ip_adapter_image_embeds=emb, **common)}
    secs = {m: [] for m in calls}
    for i in range(args.warmup + args.runs):
        for m in calls:                                  # alternated: both legs see the same drift of the box
            _, s, _ = calls[m]()
            if i >= args.warmup:
                secs[m].append(s)
    res.update(ddim_steps=args.ddim_steps, runs=args.runs, warmup=args.warmup,
               loop_seconds={m: {"min": min(v), "median": sorted(v)[len(v) // 2], "all": v} for m, v in secs.items()})
    res["image_prompt_over_plain_median"] = res["loop_seconds"]["image_prompt"]["median"] / res["loop_seconds"]["plain"]["median"]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
