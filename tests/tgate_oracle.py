"""T-GATE (Zhang et al. 2024) restated on the torch oracle: TEST INFRASTRUCTURE.

Semantics.  A *capturing* forward runs the plain UNet and stores, per transformer block, ``y`` = the output of ``attn2`` after
``to_out`` and its bias (before the residual add): the mean of the CFG pair's two halves, ``(y_uncond + y_cond) / 2``, or ``y``
itself without CFG.  A *gated* forward runs on the latents alone and every block computes ``h2 = h1 + cache`` in place of
``norm2`` and ``attn2``; it reads no prompt context.

``patched(state)`` replaces ``oracle.unet._attention`` for the duration of a forward.  ``transformer_block`` of ``oracle.unet``
-- which ``tests.sd2_oracle`` runs too, with its own head counts -- and of ``tests.tome_oracle`` look the function up in
``oracle.unet``, so one patch covers all three.  The hook acts on ``attn2`` prefixes only.
"""
from __future__ import annotations

import contextlib

import torch

UNET_TOL = 2e-2                     # tests/test_unet_gpu.py
FLOOR = 3 * UNET_TOL                # what the oracle's own distances must exceed (tests/test_tgate_cpu.py)
CACHE_TOL = 1e-2

#         id                   env          h   w  lb  cfg    seed  t0     t1
CASES = [("sd15-16x16", "sd15", 16, 16, 2, True, 29, 981.0, 961.0),             # two-GEMM and plain forms at 256 / 64 / 16 / 4 tokens
         ("sd15-16x24", "sd15", 16, 24, 2, True, 29, 981.0, 961.0),             # non-square
         ("two_level-32x32", "two_level", 32, 32, 2, True, 7, 501.0, 481.0),    # 1024 tokens: the one-launch fused form
         ("sd2-16x16", "sd2", 16, 16, 2, True, 29, 981.0, 961.0),               # 5 / 10 / 20 heads
         ("sd15-16x16-nocfg", "sd15", 16, 16, 2, False, 29, 981.0, 961.0)]      # pair = 1
VARIANTS = ("zero", "cond", "uncond", "swapped")


class TGateState:
    """``mode``: None (plain), "capture" or "reuse".  A capture fills ``cache`` / ``y_u`` / ``y_c`` per attn2 prefix, in the
    order the blocks run (``order``); ``variant`` (reuse): what is returned in place of the cache -- None = the cache."""

    def __init__(self, pair: int):
        self.pair, self.mode, self.variant = pair, None, None
        self.cache, self.y_u, self.y_c, self.order = {}, {}, {}, []

    def read(self, p: str) -> torch.Tensor:
        c = self.cache[p]
        if self.variant is None:
            return c
        if self.variant == "zero":
            return torch.zeros_like(c)
        if self.variant == "cond":
            return self.y_c[p]
        if self.variant == "uncond":
            return self.y_u[p]
        if self.variant == "swapped":      # the cache rows of the samples exchanged
            return c.flip(0)
        raise ValueError(self.variant)


@contextlib.contextmanager
def patched(state: TGateState):
    import oracle.unet as ou
    orig = ou._attention

    def attention(w, p, x, ctx, heads, fq=None):
        if not p.endswith("attn2.") or state.mode is None:
            return orig(w, p, x, ctx, heads, fq)
        if state.mode == "reuse":
            c = state.read(p)
            assert c.shape == x.shape, (p, tuple(c.shape), tuple(x.shape))
            return c
        y = orig(w, p, x, ctx, heads, fq)
        if state.pair == 2:
            u, c = y.chunk(2)
            state.y_u[p], state.y_c[p] = u, c
            state.cache[p] = (u + c) / 2
        else:
            state.y_u[p] = state.y_c[p] = state.cache[p] = y
        state.order.append(p)
        return y
    ou._attention = attention
    try:
        yield
    finally:
        ou._attention = orig


def unet_forward(w, cfg, sample, t, ctx, state: TGateState, mode, heads_per_level=None, variant=None, **kw):
    """eps of the oracle UNet with the T-GATE hook in ``mode`` (``heads_per_level``: the SD 2.x-shaped oracle)."""
    state.mode, state.variant = mode, variant
    try:
        with patched(state), torch.no_grad():
            if heads_per_level is not None:
                from tests.sd2_oracle import sd2_unet_forward
                return sd2_unet_forward(w, cfg, heads_per_level, sample, t, ctx, **kw)
            import oracle.unet as ou
            return ou.unet_forward(w, cfg, sample, t, ctx, **kw)
    finally:
        state.mode, state.variant = None, None


def block_prefixes(cfg):
    """attn2 prefixes of the library's transformer blocks in plan order (down, mid, up): the order of the cache slices."""
    nl, out = len(cfg.block_out_channels), []
    for i in range(nl):
        if cfg.attn_levels[i]:
            out += [f"down_blocks.{i}.attentions.{j}." for j in range(cfg.layers_per_block)]
    out.append("mid_block.attentions.0.")
    for i in range(nl):
        if cfg.attn_levels[nl - 1 - i]:
            out += [f"up_blocks.{i}.attentions.{j}." for j in range(cfg.layers_per_block + 1)]
    return [p + "transformer_blocks.0.attn2." for p in out]


_ENVS, _REF = {}, {}          # per UNet its weights; per case the oracle's forwards: computed once per process, never modified


def env(name: str):
    from tests.tome_oracle import unet_env
    if name not in _ENVS:
        _ENVS[name] = unet_env(name)
    return _ENVS[name]


def inputs(case):
    """(lat0 [lb], lat1 [lb], context [pair * lb] = [uncond | cond]): the capture runs on cat([lat0] * pair) at t0, the gated
    forward on lat1 at t1 -- other latents and another timestep, so that a stale h1 shows."""
    _, name, h, w, lb, cfg_on, seed, _, _ = case
    cfg = env(name)[0]
    g = torch.Generator().manual_seed(seed)
    lat0 = torch.randn(lb, 4, h, w, generator=g)
    ctx = torch.randn((2 if cfg_on else 1) * lb, cfg.context_len, cfg.cross_attention_dim, generator=g)
    lat1 = torch.randn(lb, 4, h, w, generator=torch.Generator().manual_seed(seed + 1))
    return lat0, lat1, ctx


def reference(case):
    """dict(capture = eps of the capturing forward (the plain oracle: the hook only records), gated = eps of the gated forward,
    state = the TGateState with the oracle's cache), cached."""
    key = case[0]
    if key not in _REF:
        _, name, h, w, lb, cfg_on, seed, t0, t1 = case
        cfg, sd, ocfg, heads = env(name)
        lat0, lat1, ctx = inputs(case)
        pair = 2 if cfg_on else 1
        st = TGateState(pair)
        cap = unet_forward(sd, ocfg, torch.cat([lat0] * pair), t0, ctx, st, "capture", heads_per_level=heads)
        gated = unet_forward(sd, ocfg, lat1, t1, ctx[-lb:], st, "reuse", heads_per_level=heads)
        _REF[key] = dict(capture=cap, gated=gated, state=st)
    return _REF[key]


def variant_forward(case, variant):
    """eps of the gated forward with ``variant`` in place of the cache; ``"plain"``: the plain oracle on (lat1, t1, cond rows)."""
    _, name, h, w, lb, cfg_on, seed, t0, t1 = case
    cfg, sd, ocfg, heads = env(name)
    _, lat1, ctx = inputs(case)
    st = reference(case)["state"]
    if variant == "plain":
        return unet_forward(sd, ocfg, lat1, t1, ctx[-lb:], st, None, heads_per_level=heads)
    return unet_forward(sd, ocfg, lat1, t1, ctx[-lb:], st, "reuse", heads_per_level=heads, variant=variant)


def sample_loop(weights, cfg, scheduler, prompt_embeds, negative_prompt_embeds, latents, num_inference_steps, guidance_scale,
                gate_step, heads_per_level=None):
    """``oracle.pipeline.sample_loop`` with a gate: steps 0 .. g - 1 as there (step g - 1 captures), steps g .. N - 1 run the
    gated UNet on the latents alone and hand its output to the scheduler as it is.  Returns the final latents."""
    do_cfg = guidance_scale > 1.0
    ctx = torch.cat([negative_prompt_embeds, prompt_embeds]) if do_cfg else prompt_embeds
    scheduler.set_timesteps(num_inference_steps)
    ts = list(scheduler.timesteps)
    latents = latents.float() * scheduler.init_noise_sigma
    lb = latents.shape[0]
    st = TGateState(2 if do_cfg else 1)
    g = gate_step if gate_step < len(ts) else None
    for i, t in enumerate(ts):
        if g is not None and i >= g:
            x = scheduler.scale_model_input(latents, t)
            noise_pred = unet_forward(weights, cfg, x, t, ctx[-lb:], st, "reuse", heads_per_level=heads_per_level)
        else:
            x = scheduler.scale_model_input(torch.cat([latents] * 2) if do_cfg else latents, t)
            mode = "capture" if g is not None and i == g - 1 else None
            noise_pred = unet_forward(weights, cfg, x, t, ctx, st, mode, heads_per_level=heads_per_level)
            if do_cfg:
                u, c = noise_pred.chunk(2)
                noise_pred = u + guidance_scale * (c - u)
        latents = scheduler.step(noise_pred, t, latents, return_dict=False)[0]
    return latents
