"""What self-attention guidance costs (profiles/sag_notes.md): the SAG step -- the CFG forward with the mass capture, the degrade
pass, the forward on the degraded latents at the latent batch, the step kernel -- against the plain CFG step on the same build,
the two SAG kernels' own times, launches per step, and the 50-step DDIM loop in images/s with and without SAG.  One process.

    python tools/sag_profile.py --size 64 --batch 8                       # 512 px, 8 latents: UNet batch 16, then 8
    python tools/sag_profile.py --size 64 --batch 8 --ddim-steps 0        # steps only

Synthetic SD-1.5-shaped weights, seeded inputs, DDIM, CFG 7.5, SAG scale 0.75.  Step times are free-running (no per-launch
events), the plain and the SAG step alternated inside every round so that both see the same drift of the box; the per-op figures
come from one forward with an event per launch (each reading carries ~4-5 us of launch latency that a free-running stream hides);
the two SAG kernels are also timed on their own, back to back, with one event pair round many launches.  Loop seconds are the
pipeline's own (device-synchronised wall clock of the denoising loop)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=64, help="latent side (64 = 512 px)")
    ap.add_argument("--batch", type=int, default=8, help="latent batch")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=10, help="steps per reading")
    ap.add_argument("--ddim-steps", type=int, default=50)
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=1)
    args = ap.parse_args()

    import torch
    from sonicdiffusionbayeslab_amd.models import StableDiffusionModel
    from sonicdiffusionbayeslab_amd.registry import schedulers_registry
    from sonicdiffusionbayeslab_amd.schedulers import sag_degrade
    from sonicdiffusionbayeslab_amd.weights import UNetConfig, make_synthetic_state_dict
    if not torch.cuda.is_available():
        raise SystemExit("sag_profile needs an MI355X: no GPU, no number")
    S, B = args.size, args.batch
    cfg = UNetConfig(sample_size=S)
    model = StableDiffusionModel(unet_config=cfg, state_dict=make_synthetic_state_dict(cfg, seed=1234)).to("cuda:0")
    sched = model.scheduler = schedulers_registry["ddim_scheduler"].from_config(model.scheduler.config)
    sched.set_timesteps(50, device="cuda")
    t = sched._timesteps_list[25]
    a_t = float(sched.alphas_cumprod[int(t)])
    g = torch.Generator().manual_seed(29)
    pe, ne = torch.randn(B, 77, 768, generator=g), torch.randn(B, 77, 768, generator=g)
    lat = torch.randn(B, 4, S, S, generator=g)
    net, x = model.unet, lat.cuda()
    net.set_deepcache(-1)
    mh, mw = net.sag_mid_grid(cfg, S, S)
    mass = torch.zeros(2 * B, mh * mw, device="cuda")
    eps = torch.empty(3 * B, 4, S, S, device="cuda")
    x_deg = torch.empty_like(x)
    ctx = torch.cat([ne, pe]).cuda()

    def timed(fn, n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(n):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / n

    def plain_step():
        net.forward_latents(x, 2 * B, float(t), out=eps[:2 * B])
        sched.step_fused(eps[:2 * B], 7.5, x, t, cfg=True)

    def sag_step():
        net.set_sag(True)
        net.forward_latents(x, 2 * B, float(t), out=eps[:2 * B])
        sag_degrade(x, eps[:B], mass, mh, mw, "epsilon", a_t, out=x_deg)
        net.set_sag(False)
        net.forward_latents(x_deg, B, float(t), out=eps[2 * B:], sag_forward=True)
        sched.step_fused(eps, 7.5, x, t, cfg=True, sag_scale=0.75)

    res = {"latent": S, "pixels": 8 * S, "batch": B, "mid_grid": [mh, mw], "timestep": int(t)}
    # one forward of each kind with an event per launch: launches and the capture kernel's own reading
    net.set_context(ctx)
    for _ in range(2):
        prof_plain = net.forward_profiled(x, 2 * B, float(t))
    net.set_sag(True, mass)
    net.set_context(ctx)
    net.set_sag_context(ctx[:B])
    for _ in range(2):
        prof_cap = net.forward_profiled(x, 2 * B, float(t))
    net.set_sag(False)
    launches = lambda p: sum(v["launches"] for v in p.values())      # noqa: E731
    res["launches"] = {"cfg_forward": launches(prof_plain), "cfg_forward_with_capture": launches(prof_cap),
                       "sag_mass_event_ms": prof_cap["sag_mass"]["ms"], "sag_mass_launches": prof_cap["sag_mass"]["launches"]}
    # the two kernels on their own, back to back
    lib, qkv_c = net._lib, 8 * 160
    qkv = (torch.randn(2 * B * mh * mw, 3 * qkv_c, generator=g) * 0.3).to(torch.bfloat16).cuda()
    from sonicdiffusionbayeslab_amd import _lib
    stream = _lib.current_stream()
    mass_fn = lambda: lib.sd_op_sag_attn_mass(stream, qkv.data_ptr(), qkv.data_ptr() + 2 * qkv_c, 3 * qkv_c, mass.data_ptr(), 2 * B, 8,      # noqa: E731
                                              mh * mw, 160, 1)
    deg_fn = lambda: sag_degrade(x, eps[:B], mass, mh, mw, "epsilon", a_t, out=x_deg)      # noqa: E731
    for fn in (mass_fn, deg_fn, plain_step):
        timed(fn, 3)
    net.set_sag(True)
    timed(sag_step, 3)
    res["kernel_ms"] = {"sag_attn_mass": sorted(timed(mass_fn, 200) for _ in range(3))[1],
                        "sag_degrade": sorted(timed(deg_fn, 200) for _ in range(3))[1]}
    res["step_ms"] = {"plain": [], "sag": []}
    for _ in range(args.rounds):
        res["step_ms"]["plain"].append(timed(plain_step, args.steps))
        res["step_ms"]["sag"].append(timed(sag_step, args.steps))
    med = {k: sorted(v)[len(v) // 2] for k, v in res["step_ms"].items()}
    res["step_ms_median"] = med
    res["sag_over_plain"] = med["sag"] / med["plain"]
    net.clear_sag()

    if args.ddim_steps > 0:
        common = dict(prompt_embeds=pe, negative_prompt_embeds=ne, latents=lat, num_inference_steps=args.ddim_steps, guidance_scale=7.5,
                      output_type="latent", collect_x0=False, height=8 * S, width=8 * S)
        secs = {"plain": [], "sag": []}
        for i in range(args.warmup + args.runs):
            for name in ("plain", "sag"):                   # alternated
                model.disable_sag()
                if name == "sag":
                    model.enable_sag(0.75)
                _, s, _ = model(**common)
                if i >= args.warmup:
                    secs[name].append(s)
        model.disable_sag()
        res["ddim"] = {"steps": args.ddim_steps, "runs": args.runs, "warmup": args.warmup,
                       "loop_seconds": {k: {"min": min(v), "median": sorted(v)[len(v) // 2], "all": v} for k, v in secs.items()},
                       "images_per_s": {k: B / sorted(v)[len(v) // 2] for k, v in secs.items()}}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
