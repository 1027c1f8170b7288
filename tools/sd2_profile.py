"""Stable Diffusion 2.x on the GPU: the head-dim-64 attention A/B and where a whole SD 2 forward spends its time
(profiles/sd2_notes.md).

    python tools/sd2_profile.py                       # both parts, one JSON line
    python tools/sd2_profile.py --part attention      # attn_kernel<64> against attn_pipe64_kernel (both denominators) at the
                                                      # SD 2 self-attention shapes of UNet batch 16
    python tools/sd2_profile.py --part forward        # a whole SD 2 forward at 64x64 and 96x96 latents: per-group breakdown
                                                      # (one event pair per launch) and the free-running forward time

Attention: Q | K | V side by side in one [tokens, 3 C] tensor, as the plan's fused projection writes them.  The three kernels
are selected per call through SD_ATTN_PIPE64 (0 = attn_kernel<64>, ones / valu = attn_pipe64_kernel with the denominator on
a third O^T tile / summed on the VALU).  Every (shape, kernel) is warmed up and its launch time estimated; then ``--rounds``
rounds, in each of which every (shape, kernel) gets one window between two device events, the kernels of a shape ALTERNATING,
with as many launches per window as make it ``--window-ms`` long.  Reported: median over the rounds, spread = max / min - 1 of
the SAME kernel's windows, and each pipelined variant's median against the general kernel's.  "Faster" means by more than
the larger of the two spreads.  TFLOP/s counts 4 B heads Nq Nk d.  Synthetic SD 2-shaped weights, seeded inputs."""
import argparse
import json
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# (label, heads, tokens) at d = 64: the 5- and 10-head levels at 512 and 768 pixels
ATTN_SHAPES = [("5 heads 4096x4096", 5, 4096), ("5 heads 9216x9216", 5, 9216), ("10 heads 1024x1024", 10, 1024),
               ("10 heads 2304x2304", 10, 2304)]
ATTN_KERNELS = [("general", "0"), ("pipe64_ones", "ones"), ("pipe64_valu", "valu")]


def attention_part(args):
    import torch
    from sonicdiffusionbayeslab_amd import _lib
    lib = _lib.load()
    B, d = args.unet_batch, 64
    g = torch.Generator().manual_seed(29)
    res = {}
    for label, heads, n in ATTN_SHAPES:
        C = heads * d
        qkv = torch.randn(B * n, 3 * C, generator=g).to(torch.bfloat16).cuda()
        outs = {k: torch.empty(B * n, C, dtype=torch.bfloat16, device="cuda") for k, _ in ATTN_KERNELS}

        def launch(kernel, env):
            os.environ["SD_ATTN_PIPE64"] = env
            p = qkv.data_ptr()
            _lib.check(lib.sd_op_attention(_lib.current_stream(), p, 3 * C, p + 2 * C, 3 * C, p + 4 * C, 3 * C, outs[kernel].data_ptr(), C,
                                           B, heads, n, n, d, 1.0 / math.sqrt(d)))

        def window(kernel, env, iters):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(iters):
                launch(kernel, env)
            b.record()
            torch.cuda.synchronize()
            return a.elapsed_time(b) / iters

        iters = {}
        for kernel, env in ATTN_KERNELS:           # warm-up, and the launches a window of --window-ms needs
            window(kernel, env, 5)
            iters[kernel] = max(10, int(args.window_ms / window(kernel, env, 20)))
        wins = {k: [] for k, _ in ATTN_KERNELS}
        for _ in range(args.rounds):
            for kernel, env in ATTN_KERNELS:
                wins[kernel].append(window(kernel, env, iters[kernel]))
        ref = outs["general"].float()
        row = {}
        for kernel, _ in ATTN_KERNELS:
            w = sorted(wins[kernel])
            med = w[len(w) // 2]
            row[kernel] = {"ms_median": med, "ms_min": w[0], "ms_max": w[-1], "spread": w[-1] / w[0] - 1.0, "launches_per_window": iters[kernel],
                           "window_ms": med * iters[kernel], "tflops": 4.0 * B * heads * n * n * d / (med * 1e-3) / 1e12,
                           "rel_l2_vs_general": ((outs[kernel].float() - ref).norm() / ref.norm()).item()}
        for kernel in ("pipe64_ones", "pipe64_valu"):
            row[kernel]["time_vs_general"] = row[kernel]["ms_median"] / row["general"]["ms_median"] - 1.0
        res[label] = row
        del qkv, outs
    os.environ.pop("SD_ATTN_PIPE64", None)
    return {"unet_batch": B, "rounds": args.rounds, "window_ms_target": args.window_ms, "shapes": res}


def forward_part(args):
    import torch
    from sonicdiffusionbayeslab_amd.unet import HipUNet2DConditionModel
    from sonicdiffusionbayeslab_amd.weights import make_synthetic_state_dict, sd2_unet_config
    UB = args.unet_batch
    out = {}
    sd = None
    for S in (64, 96):
        cfg = sd2_unet_config(S)
        sd = sd or make_synthetic_state_dict(cfg, seed=1234)
        net = HipUNet2DConditionModel(cfg, sd)
        g = torch.Generator().manual_seed(29)
        lat = torch.randn(UB // 2, 4, S, S, generator=g).cuda()
        ctx = torch.randn(UB, cfg.context_len, cfg.cross_attention_dim, generator=g).cuda()
        net.set_context(ctx)
        for _ in range(2):
            prof = net.forward_profiled(lat, UB, 501.0)
        for _ in range(3):
            net.forward_latents(lat, UB, 501.0)
        torch.cuda.synchronize()
        wins = []
        for _ in range(args.rounds):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(args.forwards):
                net.forward_latents(lat, UB, 501.0)
            b.record()
            torch.cuda.synchronize()
            wins.append(a.elapsed_time(b) / args.forwards)
        wins.sort()
        total = sum(v["ms"] for v in prof.values())
        out[f"{S}x{S}"] = {
            "forward_ms_median": wins[len(wins) // 2], "forward_ms_all": wins, "window_ms": wins[len(wins) // 2] * args.forwards,
            "per_launch_event_ms_total": total, "launches": sum(v["launches"] for v in prof.values()),
            "groups": {k: {"ms": v["ms"], "share": v["ms"] / total, "launches": v["launches"],
                           "tflops": (v["flops"] / (v["ms"] * 1e-3) / 1e12) if v["ms"] > 0 else 0.0}
                       for k, v in sorted(prof.items(), key=lambda kv: -kv[1]["ms"]) if v["launches"]}}
        del net
        torch.cuda.empty_cache()
    return {"unet_batch": UB, "forwards_per_window": args.forwards, "rounds": args.rounds, "sizes": out}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=["all", "attention", "forward"], default="all")
    ap.add_argument("--unet-batch", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=400.0, help="length of one timed attention window")
    ap.add_argument("--forwards", type=int, default=5, help="forwards per timed window")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("sd2_profile needs an MI355X: no GPU, no number")
    res = {}
    if args.part in ("all", "attention"):
        res["attention"] = attention_part(args)
    if args.part in ("all", "forward"):
        res["forward"] = forward_part(args)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
