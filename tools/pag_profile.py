"""What perturbed-attention guidance costs (profiles/pag_notes.md): the forward at three copies of the latents with PAG on a few
layer sets against the plain forwards at two and at three copies, launches per forward, the identity op's time, and the 50-step
DDIM loop in images/s with and without PAG.  One process.

    python tools/pag_profile.py --size 64 --batch 8                       # 512 px, 8 latents: UNet batch 24 (PAG) / 16 (CFG)
    python tools/pag_profile.py --size 64 --batch 8 --ddim-steps 0        # forwards only

A setting is ``plain:R`` (the plain plan at R copies of the latents, 2 = the CFG pair, 3 = a batch as large as PAG's) or
``pag:NAMES`` with NAMES = ``mid``, ``rest`` (every transformer block but the first, fifteen of SD 1.5's sixteen: the prefix
rule does not apply), ``all``, or names joined by ``+`` in diffusers' spelling.  Synthetic SD-1.5-shaped weights, seeded inputs, DDIM, CFG 7.5, PAG scale 3.  Forward times are
free-running (no per-launch events), the settings alternated inside every round so that all see the same drift of the box; the
per-op figures come from one forward with an event per launch (each reading carries ~4-5 us of launch latency that a
free-running stream hides).  Loop seconds are the pipeline's own (device-synchronised wall clock of the denoising loop)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

OPS = ("pag_identity", "attention", "gemm", "layernorm", "groupnorm", "xattn_fused", "replicate", "conv3x3")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=64, help="latent side (64 = 512 px)")
    ap.add_argument("--batch", type=int, default=8, help="latent batch")
    ap.add_argument("--settings", nargs="+", default=["plain:2", "plain:3", "pag:mid", "pag:rest"])
    ap.add_argument("--loop-settings", nargs="*", default=["plain:2", "pag:mid"], help="settings of the DDIM loop")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--forwards", type=int, default=10)
    ap.add_argument("--ddim-steps", type=int, default=50)
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=1)
    args = ap.parse_args()

    import torch
    from sonicdiffusionbayeslab_amd.models import StableDiffusionModel
    from sonicdiffusionbayeslab_amd.registry import schedulers_registry
    from sonicdiffusionbayeslab_amd.unet import HipUNet2DConditionModel as U
    from sonicdiffusionbayeslab_amd.weights import UNetConfig, make_synthetic_state_dict
    if not torch.cuda.is_available():
        raise SystemExit("pag_profile needs an MI355X: no GPU, no number")
    S, B = args.size, args.batch
    cfg = UNetConfig(sample_size=S)
    model = StableDiffusionModel(unet_config=cfg, state_dict=make_synthetic_state_dict(cfg, seed=1234)).to("cuda:0")
    model.scheduler = schedulers_registry["ddim_scheduler"].from_config(model.scheduler.config)
    g = torch.Generator().manual_seed(29)
    pe, ne = torch.randn(B, 77, 768, generator=g), torch.randn(B, 77, 768, generator=g)
    lat = torch.randn(B, 4, S, S, generator=g)
    net, x = model.unet, lat.cuda()
    net.set_deepcache(-1)
    names = U.pag_block_names(cfg)

    def layers(spec):
        return {"mid": ["mid"], "rest": names[1:], "all": names}.get(spec) or spec.split("+")

    def setup(name):
        """-> the UNet batch of the setting, the handle ready for its forwards"""
        kind, arg = name.split(":")
        rep = int(arg) if kind == "plain" else 3
        net.set_pag(U.pag_layer_mask(cfg, layers(arg)) if kind == "pag" else 0)
        net.set_context(torch.cat([ne, pe, pe][:rep]).cuda())
        return rep * B

    res = {"latent": S, "pixels": 8 * S, "batch": B, "settings": {}}
    for name in args.settings:         # one forward with an event per launch: launches and milliseconds per op kind
        ub = setup(name)
        for _ in range(2):
            prof = net.forward_profiled(x, ub, 501.0)
        res["settings"][name] = {
            "unet_batch": ub, "launches": sum(v["launches"] for v in prof.values()),
            "per_launch_event_ms_total": sum(v["ms"] for v in prof.values()),
            "op_ms": {k: prof[k]["ms"] for k in OPS if k in prof}, "op_launches": {k: prof[k]["launches"] for k in OPS if k in prof},
            "identity_bytes": prof["pag_identity"]["bytes"] if "pag_identity" in prof else 0, "forward_ms": []}
    for _ in range(args.rounds):       # free-running forwards, the settings alternated
        for name in args.settings:
            ub = setup(name)
            for _ in range(2):
                net.forward_latents(x, ub, 501.0)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(args.forwards):
                net.forward_latents(x, ub, 501.0)
            b.record()
            torch.cuda.synchronize()
            res["settings"][name]["forward_ms"].append(a.elapsed_time(b) / args.forwards)
    base = sorted(res["settings"][args.settings[0]]["forward_ms"])[args.rounds // 2]
    for r in res["settings"].values():
        r["forward_ms_median"] = sorted(r["forward_ms"])[args.rounds // 2]
        r["forward_over_first_setting"] = r["forward_ms_median"] / base
    net.set_pag(0)

    if args.loop_settings and args.ddim_steps > 0:
        common = dict(prompt_embeds=pe, negative_prompt_embeds=ne, latents=lat, num_inference_steps=args.ddim_steps, guidance_scale=7.5,
                      output_type="latent", collect_x0=False, height=8 * S, width=8 * S)
        secs = {name: [] for name in args.loop_settings}
        for i in range(args.warmup + args.runs):
            for name in args.loop_settings:                 # alternated
                kind, arg = name.split(":")
                model.disable_pag()
                if kind == "pag":
                    model.enable_pag(pag_scale=3.0, pag_applied_layers=layers(arg))
                elif arg != "2":
                    continue
                _, s, _ = model(**common)
                if i >= args.warmup:
                    secs[name].append(s)
        model.disable_pag()
        secs = {k: v for k, v in secs.items() if v}
        res["ddim"] = {"steps": args.ddim_steps, "runs": args.runs, "warmup": args.warmup,
                       "loop_seconds": {k: {"min": min(v), "median": sorted(v)[len(v) // 2], "all": v} for k, v in secs.items()},
                       "images_per_s": {k: B / sorted(v)[len(v) // 2] for k, v in secs.items()}}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
