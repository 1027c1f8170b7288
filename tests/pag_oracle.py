"""Perturbed-attention guidance (PAG; Ahn et al. 2024, diffusers' ``PAGMixin``) restated on the torch oracle:
TEST INFRASTRUCTURE (upstream-recall, no upstream text).

Semantics.  One set of ``lb`` latents; the UNet batch is ``[uncond | cond | perturbed]`` (``ub = 3 lb``, prompt rows
``[neg | pos | pos]``) with CFG and ``[cond | perturbed]`` (``ub = 2 lb``) without; the perturbed samples are the last ``lb``.
In a transformer block named by ``pag_applied_layers`` the self-attention of a perturbed sample is
``to_out(to_v(norm1(h)))`` -- no scores, no softmax, the same weights and bias; ``attn2``, the feed-forward and every other
block are untouched.  Guidance per element: ``e = (u + g (c - u)) + s (c - p)`` with CFG, ``e = c + s (c - p)`` without;
``s_t = pag_scale`` or ``max(pag_scale - pag_adaptive_scale (1000 - t), 0)``; ``guidance_rescale`` is
``rescale_noise_cfg(e, c, r)`` with ``e`` including the PAG term, with CFG only.

``patched(run)`` puts ``attention`` below in place of ``oracle.unet._attention`` -- looked up through the module by
``oracle.unet.transformer_block`` (which ``tests.sd2_oracle`` runs too) and by ``tests.hypertile_oracle.transformer_block``,
so the HyperTile oracle composes: its tiles are samples, and the perturbed ones stay last.
"""
from __future__ import annotations

import contextlib

import torch
import torch.nn.functional as F

UNET_TOL = 2e-2                     # tests/test_unet_gpu.py
FLOOR = 5 * UNET_TOL                # what the oracle's own perturbed-against-cond distance must exceed at every UNet case


def block_prefixes(cfg):
    """[(diffusers' PAG name, state-dict prefix)] of the transformer blocks in call order (down, mid, up), from the config."""
    nlev = len(cfg.block_out_channels)
    out = []
    for i in range(nlev):
        if cfg.attn_levels[i]:
            out += [(f"down.block_{i}.attentions_{j}", f"down_blocks.{i}.attentions.{j}.") for j in range(cfg.layers_per_block)]
    out.append(("mid", "mid_block.attentions.0."))
    for i in range(nlev):
        if cfg.attn_levels[nlev - 1 - i]:
            out += [(f"up.block_{i}.attentions_{j}", f"up_blocks.{i}.attentions.{j}.") for j in range(cfg.layers_per_block + 1)]
    return out


def layer_bits(cfg, layers):
    """The blocks ``layers`` (a name or a list) selects, as indices into ``block_prefixes``; a name is a block's own or the part
    of it in front of ``.attentions_j``.  ``ValueError`` for a name that selects nothing."""
    names = [layers] if isinstance(layers, str) else list(layers)
    blocks = block_prefixes(cfg)
    bits = set()
    for name in names:
        hit = [k for k, (n, _) in enumerate(blocks) if n == name or n.split(".attentions_")[0] == name]
        if not hit:
            raise ValueError(name)
        bits.update(hit)
    return sorted(bits)


def layer_mask(cfg, layers) -> int:
    return sum(1 << k for k in layer_bits(cfg, layers))


def step_scale(pag_scale: float, adaptive: float, t) -> float:
    return float(pag_scale) if adaptive == 0 else max(float(pag_scale) - float(adaptive) * (1000.0 - float(t)), 0.0)


class PagRun:
    """The setting of one oracle forward: the last ``lb`` of ``ub`` samples are perturbed in the blocks ``layers`` names.
    ``used`` collects the prefix of every block that ran perturbed, in call order."""

    def __init__(self, cfg, lb: int, ub: int, layers):
        blocks = block_prefixes(cfg)
        self.lb, self.ub = lb, ub
        self.prefixes = {blocks[k][1] for k in layer_bits(cfg, layers)} if layers else set()
        self.used = []


_ORIG = {}


def attention(w, p: str, x: torch.Tensor, ctx: torch.Tensor, heads: int, fq=None, run: PagRun = None) -> torch.Tensor:
    """``oracle.unet._attention`` with the identity attention for the perturbed samples of a named block's ``attn1``."""
    tail = "transformer_blocks.0.attn1."
    if run is None or not p.endswith(tail) or p[:-len(tail)] not in run.prefixes:
        return _ORIG["attention"](w, p, x, ctx, heads, fq)
    assert fq is None, "PAG on fp8 handles is not built"
    run.used.append(p[:-len(tail)])
    n = x.shape[0] // run.ub * run.lb          # (a HyperTile block hands every tile over as a sample)
    plain = _ORIG["attention"](w, p, x[:-n], ctx[:-n], heads, fq)
    v = F.linear(ctx[-n:], w[p + "to_v.weight"])
    return torch.cat([plain, F.linear(v, w[p + "to_out.0.weight"], w[p + "to_out.0.bias"])])


@contextlib.contextmanager
def patched(run: PagRun):
    import oracle.unet as ou
    _ORIG["attention"] = ou._attention

    def att(w, p, x, ctx, heads, fq=None):
        return attention(w, p, x, ctx, heads, fq, run)
    ou._attention = att
    try:
        yield
    finally:
        ou._attention = _ORIG.pop("attention")


def unet_forward(w, cfg, sample, t, ctx, run: PagRun, heads_per_level=None, tile=None, **kw):
    """eps of the oracle UNet perturbed as ``run`` describes (``heads_per_level``: the SD 2.x-shaped oracle; ``tile``: a
    ``tests.hypertile_oracle.TileRun``)."""
    import tests.hypertile_oracle as ho
    with patched(run):
        return ho.unet_forward(w, cfg, sample, t, ctx, tile if tile is not None else ho.TileRun(tuple(sample.shape[-2:]), 0),
                               heads_per_level=heads_per_level, **kw)


def guided(eps: torch.Tensor, lb: int, cfg: bool, g: float, s: float, rescale: float = 0.0) -> torch.Tensor:
    """The prediction the step works on, from eps = [u | c | p] (``cfg``) or [c | p]."""
    if cfg:
        u, c, p = eps[:lb], eps[lb:2 * lb], eps[2 * lb:]
        e = (u + g * (c - u)) + s * (c - p)
        if rescale > 0.0:
            dims = list(range(1, e.dim()))
            e = (rescale * (c.std(dim=dims, keepdim=True) / e.std(dim=dims, keepdim=True)) + (1.0 - rescale)) * e
        return e
    c, p = eps[:lb], eps[lb:]
    return c + s * (c - p)


def context(pe, ne, cfg: bool):
    """The prompt rows of a PAG batch: [neg | pos | pos] with CFG, [pos | pos] without."""
    return torch.cat([ne, pe, pe]) if cfg else torch.cat([pe, pe])


@torch.no_grad()
def loop(w, ocfg, sched, timesteps, pe, ne, lat, gs, layers, pag_scale, adaptive=0.0, heads_per_level=None, rescale=0.0):
    """The sampling loop with PAG over ``timesteps`` of ``sched`` (an oracle scheduler whose ``set_timesteps`` has run), from the
    start latents ``lat``: final latents."""
    cfg = ne is not None
    lb = lat.shape[0]
    ctx = context(pe, ne, cfg)
    ub = ctx.shape[0]
    x = lat.float()
    for t in timesteps:
        run = PagRun(ocfg, lb, ub, layers)
        eps = unet_forward(w, ocfg, torch.cat([x] * (ub // lb)), t, ctx, run, heads_per_level=heads_per_level)
        e = guided(eps, lb, cfg, gs, step_scale(pag_scale, adaptive, t), rescale)
        x = sched.step(e, t, x, return_dict=False)[0]
    return x


#             env          h   w   lb  seed  t      layers                                    perturbed blocks
UNET_CASES = [("sd15", 16, 16, 2, 29, 981.0, ("mid", "up.block_1"), 4),
              ("sd15", 16, 16, 2, 29, 981.0, ("down.block_2", "mid", "up.block_1"), 6),
              ("sd15", 16, 16, 2, 29, 981.0, ("down.block_0.attentions_0",), 1),       # the first block: the prefix rule
              ("sd15", 16, 16, 2, 29, 981.0, ("down.block_0",), 2),
              # 32x32 latents on the 320 / 640 UNet: level 0 has 1024 tokens, the fused prompt cross-attention.  With 2 latents the
              # q|k|v projection has 6144 or 4096 rows and runs on 64-row tiles, which keep K / V token-major
              ("two_level", 32, 32, 2, 7, 501.0, ("down.block_0", "up.block_1"), 5)]
# ... with 3 latents x 3 it has 9216 rows, 128-row tiles, and stores K / V head-major: the identity op's other layout
HM_CASE = ("two_level", 32, 32, 3, 7, 501.0, ("down.block_0", "up.block_1"), 5)
SD2_CASE = ("sd2", 16, 16, 1, 29, 981.0, ("down.block_1", "mid", "up.block_2"), 6)
# HyperTile (T = 8 tokens: level 0 of a 16x16 latent runs 2x2 tiles) under the second case's layers plus a tiled perturbed block
HT_CASE = ("sd15", 16, 16, 2, 29, 981.0, ("mid", "up.block_1", "up.block_3.attentions_2"), 5)
HT_TOKENS = 8
# the default layer set moves the output less than the floor at every shape tried: it is tested at the "mid" debug tensor
MID_CASE = ("sd15", 16, 16, 2, 29, 981.0, ("mid",), 1)
MID_FLOOR = 5 * UNET_TOL


def unet_inputs(cfg, h: int, w: int, lb: int, rep: int, seed: int = 29):
    """(latents [lb], prompt rows [rep * lb], UNet sample [rep * lb]) of a UNet case at ``rep`` = 3 ([neg | pos | pos]) or 2
    ([pos | pos]): one draw per seed, so both batch forms share the latents and the positive prompt."""
    g = torch.Generator().manual_seed(seed)
    lat = torch.randn(lb, 4, h, w, generator=g)
    two = torch.randn(2 * lb, cfg.context_len, cfg.cross_attention_dim, generator=g)
    ne, pe = two[:lb], two[lb:]
    return lat, context(pe, ne if rep == 3 else None, rep == 3), torch.cat([lat] * rep)


_ENVS, _REF = {}, {}          # per UNet its weights; per case the oracle's forwards: computed once per process, never modified


def env(name: str):
    from tests.tome_oracle import unet_env
    if name not in _ENVS:
        _ENVS[name] = unet_env(name)
    return _ENVS[name]


def reference(case, rep: int = 3, tile_tokens: int = 0):
    """dict(eps = the PAG oracle's output [rep * lb], plain = the plain oracle's on the first (rep - 1) * lb samples, used = the
    perturbed blocks in call order, mid / mid_plain = the "mid" taps) at a case, cached."""
    key = (case, rep, tile_tokens)
    if key not in _REF:
        import tests.hypertile_oracle as ho
        name, h, w, lb, seed, t, layers, _ = case
        cfg, sd, ocfg, heads = env(name)
        lat, ctx, sample = unet_inputs(cfg, h, w, lb, rep, seed)
        tile = lambda: ho.TileRun((h, w), tile_tokens)
        run, taps, ptaps = PagRun(ocfg, lb, rep * lb, layers), {}, {}
        kw = {} if heads is not None else {"taps": taps}
        pkw = {} if heads is not None else {"taps": ptaps}
        with torch.no_grad():
            eps = unet_forward(sd, ocfg, sample, t, ctx, run, heads_per_level=heads, tile=tile(), **kw)
            plain = unet_forward(sd, ocfg, sample[:-lb], t, ctx[:-lb], PagRun(ocfg, lb, rep * lb, ()), heads_per_level=heads,
                                 tile=tile(), **pkw)
        _REF[key] = dict(eps=eps, plain=plain, used=run.used, mid=taps.get("mid"), mid_plain=ptaps.get("mid"))
    return _REF[key]
