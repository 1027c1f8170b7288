"""What UniPC costs and what it buys (profiles/unipc_notes.md): the step's time beside DPM-Solver++'s, images per second of whole
loops, and the solver's accuracy on the synthetic-weight UNet.

    python tools/unipc_profile.py --step                     # sd_sched_step_pc vs sd_sched_step (DPM-Solver++ 2M), same build
    python tools/unipc_profile.py --loops 10 20              # images/s, UniPC and DPM-Solver++ order 2 alternated
    python tools/unipc_profile.py --loops 10 20 --schedulers dpm     # one side only (a checkout without UniPC)
    python tools/unipc_profile.py --accuracy 8 10 15         # rel-L2 to a 200-step DPM-Solver++ result from the same noise
    python tools/unipc_profile.py --one-call 8               # one 8-step UniPC call (for rocprofv3 --kernel-trace --stats)

Synthetic SD-1.5-shaped weights, seeded inputs, 512 px, 8 latents and CFG unless told otherwise; latents out (no VAE).  The two
schedulers are alternated inside every round so that both see the same drift of the box; the first round warms up and is
dropped; medians are reported with the spread (min, max) of the repeats."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

KW = {"unipc": ("unipc_scheduler", dict(solver_order=2, solver_type="bh2")),
      "dpm": ("dpm_solver_scheduler", dict(solver_order=2, algorithm_type="dpmsolver++", final_sigmas_type="zero"))}


def stats(v):
    v = sorted(v)
    return {"median": v[len(v) // 2], "min": v[0], "max": v[-1], "n": len(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=64, help="latent side (64 = 512 px)")
    ap.add_argument("--batch", type=int, default=8, help="latents per call")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--schedulers", nargs="+", default=["unipc", "dpm"], choices=sorted(KW))
    ap.add_argument("--step", action="store_true")
    ap.add_argument("--loops", type=int, nargs="*", default=[])
    ap.add_argument("--accuracy", type=int, nargs="*", default=[])
    ap.add_argument("--reference-steps", type=int, default=200)
    ap.add_argument("--one-call", type=int, default=None)
    args = ap.parse_args()

    import torch
    from sonicdiffusionbayeslab_amd.models import StableDiffusionModel
    from sonicdiffusionbayeslab_amd.registry import schedulers_registry
    from sonicdiffusionbayeslab_amd.schedulers import PNDMConfigStub
    from sonicdiffusionbayeslab_amd.weights import UNetConfig, make_synthetic_state_dict
    if not torch.cuda.is_available():
        raise SystemExit("unipc_profile needs an MI355X: no GPU, no number")
    S, B = args.size, args.batch

    def sched(kind, **more):
        name, kw = KW[kind]
        return schedulers_registry[name].from_config(PNDMConfigStub().config, **dict(kw, **more))

    res = {"latent_side": S, "latents": B, "rounds": args.rounds}
    g = torch.Generator().manual_seed(29)

    if args.step:                          # the step alone: random [u | c] model outputs, every step of a 20-step schedule
        shape = (B, 4, S, S)
        x = torch.randn(shape, generator=g).cuda()
        e2 = torch.randn((2 * B,) + shape[1:], generator=g).cuda()
        times = {k: [] for k in args.schedulers}
        for rnd in range(args.rounds + 1):
            for kind in args.schedulers:
                s = sched(kind)
                s.set_timesteps(20, device="cuda")
                ts = list(s._timesteps_list)
                for t in ts[:3]:           # (fills the history: the timed steps run at full order)
                    s.step_fused(e2, 7.5, x, t, cfg=True)
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for t in ts[3:19]:
                    s.step_fused(e2, 7.5, x, t, cfg=True)
                b.record()
                torch.cuda.synchronize()
                if rnd:
                    times[kind].append(a.elapsed_time(b) * 1e3 / 16)
        res["step_us"] = {k: stats(v) for k, v in times.items()}

    if args.loops or args.accuracy or args.one_call:
        cfg = UNetConfig(sample_size=S)
        sd = make_synthetic_state_dict(cfg, seed=1234)
        model = StableDiffusionModel(unet_config=cfg, state_dict=sd).to("cuda:0")
        lat = torch.randn(B, 4, S, S, generator=g)
        pe, ne = torch.randn(B, 77, 768, generator=g), torch.randn(1, 77, 768, generator=g).repeat(B, 1, 1)

        def call(kind, n, lat=lat, pe=pe, ne=ne, **more):
            model.scheduler = sched(kind, **more)
            out, secs, _ = model(prompt_embeds=pe, negative_prompt_embeds=ne, latents=lat, num_inference_steps=n,
                                 guidance_scale=7.5, output_type="latent", collect_x0=False)
            return out.images, secs

        if args.one_call:
            call(args.schedulers[0], args.one_call)
            torch.cuda.synchronize()
            print(json.dumps({"one_call": args.one_call, "scheduler": args.schedulers[0]}))
            return
        if args.loops:
            res["loops"] = {}
            for n in args.loops:
                secs = {k: [] for k in args.schedulers}
                for rnd in range(args.rounds + 1):
                    for kind in args.schedulers:
                        s = call(kind, n)[1]
                        if rnd:
                            secs[kind].append(s)
                ips = {k: stats([B / s for s in v]) for k, v in secs.items()}
                res["loops"][str(n)] = {"images_per_s": ips}
                if len(args.schedulers) == 2:
                    a, b = args.schedulers
                    res["loops"][str(n)][f"{a}_over_{b}"] = ips[a]["median"] / ips[b]["median"]
        if args.accuracy:                  # two latents are enough for a distance
            l2, p2, n2 = lat[:2], pe[:2], ne[:2]
            ref = call("dpm", args.reference_steps, l2, p2, n2)[0].double().cpu()
            res["accuracy"] = {"reference": f"dpm order 2, {args.reference_steps} steps", "rel_l2": {}}
            for n in args.accuracy:
                row = {}
                for kind in args.schedulers:
                    got = call(kind, n, l2, p2, n2)[0].double().cpu()
                    row[kind] = ((got - ref).norm() / ref.norm()).item()
                res["accuracy"]["rel_l2"][str(n)] = row
    print(json.dumps(res))


if __name__ == "__main__":
    main()
