"""What T-GATE saves (profiles/tgate_notes.md): milliseconds per UNet forward of the four plans a gated run uses, their launch
counts, and images per second of whole DDIM loops with and without a gate.

    python tools/tgate_profile.py                          # 512 px, 8 latents (UNet batch 16 under CFG)
    python tools/tgate_profile.py --loops 25 50 --gate 10   # also the sampling loops (latents out: no VAE)
    python tools/tgate_profile.py --one-forward gated       # one forward of one plan (for rocprofv3 --kernel-trace --stats)

Synthetic SD-1.5-shaped weights, seeded inputs.  All plans are the SAME build, the same process and the same handle: the plain
CFG plan (UNet batch 2 B), the plain non-CFG plan (B), the capture plan (2 B) and the gated plan (B).  Forward times are
free-running (no per-launch events) and the four plans are alternated inside every round, so that all see the same drift of the
box; the median over the rounds is reported with all readings.  Launch counts come from one forward with an event per launch.
The gated plan reads the cache the capture plan of the same round filled."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PLANS = ("plain_cfg", "plain_nocfg", "capture", "gated")
OPS = ("tgate_capture", "tgate_apply", "tgate_zero", "xattn_fused", "attention", "gemm", "layernorm")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=64, help="latent side (64 = 512 px)")
    ap.add_argument("--batch", type=int, default=8, help="latents per call")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--forwards", type=int, default=10)
    ap.add_argument("--loops", type=int, nargs="*", default=[], help="DDIM step counts to time whole loops at")
    ap.add_argument("--gate", type=int, default=10)
    ap.add_argument("--one-forward", choices=PLANS, default=None)
    args = ap.parse_args()

    import torch
    from sonicdiffusionbayeslab_amd.unet import HipUNet2DConditionModel
    from sonicdiffusionbayeslab_amd.weights import UNetConfig, make_synthetic_state_dict
    if not torch.cuda.is_available():
        raise SystemExit("tgate_profile needs an MI355X: no GPU, no number")
    S, B = args.size, args.batch
    cfg = UNetConfig(sample_size=S)
    sd = make_synthetic_state_dict(cfg, seed=1234)
    net = HipUNet2DConditionModel(cfg, sd)
    g = torch.Generator().manual_seed(29)
    ctx2 = torch.randn(2 * B, 77, 768, generator=g).cuda()
    ctx1 = ctx2[B:].contiguous()
    x = torch.randn(B, 4, S, S, generator=g).cuda()
    net.set_deepcache(-1)
    net.reserve_tgate(B)
    eps = {2 * B: torch.empty(2 * B, 4, S, S, device="cuda"), B: torch.empty(B, 4, S, S, device="cuda")}

    def setup(plan):
        """The handle state and the context of a plan; returns its UNet batch."""
        if plan == "gated":            # (needs the capture of this round)
            net.set_tgate(net.TGATE_REUSE, B)
            return B
        net.set_tgate(net.TGATE_CAPTURE, B) if plan == "capture" else net.set_tgate(net.TGATE_OFF)
        ub = B if plan == "plain_nocfg" else 2 * B
        net.set_context(ctx1 if ub == B else ctx2)
        return ub

    res = {"latent_side": S, "latents": B, "rounds": args.rounds, "forwards": args.forwards, "plans": {}}
    try:
        if args.one_forward:
            if args.one_forward == "gated":
                ub = setup("capture")
                net.forward_latents(x, ub, 501.0, out=eps[ub])
            ub = setup(args.one_forward)
            net.forward_latents(x, ub, 481.0, out=eps[ub])
            torch.cuda.synchronize()
            print(json.dumps({"one_forward": args.one_forward, "unet_batch": ub}))
            return
        out = {p: {"forward_ms": []} for p in PLANS}
        for p in PLANS:                    # one forward with an event per launch: launches per op kind
            ub = setup(p)
            for _ in range(2):
                prof = net.forward_profiled(x, ub, 501.0)
            out[p].update(unet_batch=ub, launches=sum(v["launches"] for v in prof.values()),
                          per_launch_event_ms_total=sum(v["ms"] for v in prof.values()),
                          op_launches={k: prof[k]["launches"] for k in OPS if k in prof},
                          op_ms={k: prof[k]["ms"] for k in OPS if k in prof})
        for _ in range(args.rounds):       # free-running forwards, the four plans alternated
            for p in PLANS:
                ub = setup(p)
                for _ in range(3):
                    net.forward_latents(x, ub, 501.0, out=eps[ub])
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(args.forwards):
                    net.forward_latents(x, ub, 501.0, out=eps[ub])
                b.record()
                torch.cuda.synchronize()
                out[p]["forward_ms"].append(a.elapsed_time(b) / args.forwards)
        for p in PLANS:
            v = sorted(out[p]["forward_ms"])
            out[p]["forward_ms_median"], out[p]["forward_ms_min"], out[p]["forward_ms_max"] = v[len(v) // 2], v[0], v[-1]
        out["gated_over_plain_nocfg"] = out["gated"]["forward_ms_median"] / out["plain_nocfg"]["forward_ms_median"]
        out["gated_over_plain_cfg"] = out["gated"]["forward_ms_median"] / out["plain_cfg"]["forward_ms_median"]
        out["capture_over_plain_cfg"] = out["capture"]["forward_ms_median"] / out["plain_cfg"]["forward_ms_median"]
        res["plans"] = out
    finally:
        net.set_tgate(net.TGATE_OFF)
        net.reserve_tgate(None)
    del net
    torch.cuda.empty_cache()

    if args.loops:                         # whole DDIM loops through the pipeline, latents out, gate off and on alternated
        from sonicdiffusionbayeslab_amd.models import StableDiffusionModel
        from sonicdiffusionbayeslab_amd.registry import schedulers_registry
        model = StableDiffusionModel(unet_config=cfg, state_dict=sd).to("cuda:0")
        model.scheduler = schedulers_registry["ddim_scheduler"].from_config(model.scheduler.config)
        pe, ne = ctx2[B:].cpu(), ctx2[:B].cpu()
        lat = x.cpu()
        res["loops"] = {}
        for n in args.loops:
            r = {"off": [], "on": []}
            for rnd in range(args.rounds + 1):            # (the first round warms both up and is dropped)
                for mode in ("off", "on"):
                    model.enable_tgate(args.gate) if mode == "on" else model.disable_tgate()
                    torch.cuda.synchronize()
                    t0 = time.time()
                    _, secs, _ = model(prompt_embeds=pe, negative_prompt_embeds=ne, latents=lat, num_inference_steps=n,
                                       guidance_scale=7.5, output_type="latent", collect_x0=False)
                    torch.cuda.synchronize()
                    if rnd:
                        r[mode].append({"loop_s": secs, "call_s": time.time() - t0})
            model.disable_tgate()
            med = {m: sorted(v["loop_s"] for v in r[m])[len(r[m]) // 2] for m in r}
            res["loops"][str(n)] = {"gate": args.gate, "readings": r, "images_per_s": {m: B / med[m] for m in med},
                                    "on_over_off_images_per_s": med["off"] / med["on"]}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
