"""What FreeU costs (profiles/freeu_notes.md): the UNet forward with FreeU off and on at several image sizes, and the launch
counts and per-launch-event times of the op kinds it touches.

    python tools/freeu_profile.py                          # 512, 768 and 1024 px at UNet batch 16
    python tools/freeu_profile.py --sizes 64 --plain-only   # the off path alone (runs on a build without FreeU as well)

Synthetic SD-1.5-shaped weights, seeded inputs.  Off and on are the SAME build and the same handle; forward times are
free-running (no per-launch events), off and on alternated inside every round so that both see the same drift of the box, the
median over the rounds reported with all readings.  The per-op figures come from one forward with an event per launch (each
reading carries ~4-5 us of launch latency that a free-running stream hides).  ``--plain-only`` touches no FreeU entry point:
copied into a checkout of an earlier commit it times that commit's plain forward with the same method."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

OPS = ("freeu", "groupnorm", "conv3x3", "gemm")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[64, 96, 128], help="latent sides (64 = 512 px)")
    ap.add_argument("--unet-batch", type=int, default=16)
    ap.add_argument("--factors", type=float, nargs=4, default=[0.9, 0.2, 1.5, 1.6], metavar=("S1", "S2", "B1", "B2"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--forwards", type=int, default=10)
    ap.add_argument("--plain-only", action="store_true")
    args = ap.parse_args()

    import torch
    from sonicdiffusionbayeslab_amd.unet import HipUNet2DConditionModel
    from sonicdiffusionbayeslab_amd.weights import UNetConfig, make_synthetic_state_dict
    if not torch.cuda.is_available():
        raise SystemExit("freeu_profile needs an MI355X: no GPU, no number")
    UB = args.unet_batch
    modes = ["off"] if args.plain_only else ["off", "on"]
    res = {"unet_batch": UB, "factors": None if args.plain_only else args.factors, "rounds": args.rounds, "forwards": args.forwards,
           "sizes": {}}
    sd = None
    for S in args.sizes:
        cfg = UNetConfig(sample_size=S)
        if sd is None:
            sd = make_synthetic_state_dict(cfg, seed=1234)
        net = HipUNet2DConditionModel(cfg, sd)
        g = torch.Generator().manual_seed(29)
        ctx = torch.randn(UB, 77, 768, generator=g).cuda()
        x = torch.randn(UB // 2, 4, S, S, generator=g).cuda()          # a CFG pair: the UNet batch is twice the latent batch
        net.set_deepcache(-1)

        def setup(mode):
            if not args.plain_only:
                if mode == "on":
                    net.set_freeu(*args.factors)
                else:
                    net.disable_freeu()
            net.set_context(ctx)

        out = {m: {"forward_ms": []} for m in modes}
        for m in modes:                    # one forward with an event per launch: launches and milliseconds per op kind
            setup(m)
            for _ in range(2):
                prof = net.forward_profiled(x, UB, 501.0)
            out[m].update(launches=sum(v["launches"] for v in prof.values()),
                          per_launch_event_ms_total=sum(v["ms"] for v in prof.values()),
                          op_ms={k: prof[k]["ms"] for k in OPS if k in prof},
                          op_launches={k: prof[k]["launches"] for k in OPS if k in prof})
        for _ in range(args.rounds):       # free-running forwards, off and on alternated
            for m in modes:
                setup(m)
                for _ in range(3):
                    net.forward_latents(x, UB, 501.0)
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(args.forwards):
                    net.forward_latents(x, UB, 501.0)
                b.record()
                torch.cuda.synchronize()
                out[m]["forward_ms"].append(a.elapsed_time(b) / args.forwards)
        for m in modes:
            v = sorted(out[m]["forward_ms"])
            out[m]["forward_ms_median"], out[m]["forward_ms_min"] = v[len(v) // 2], v[0]
        if "on" in out:
            out["on_over_off"] = out["on"]["forward_ms_median"] / out["off"]["forward_ms_median"]
        res["sizes"][str(8 * S)] = out
        del net
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
