"""HyperTile (tiled self-attention) restated on the torch oracle: TEST INFRASTRUCTURE.

Semantics.  ``T`` is the tile side in tokens.  A transformer block on ``rh x rw`` tokens of a ``lh x lw`` latent has depth
``d = log2(lh / rh)``; with ``d <= max_depth`` its tile side ``th`` is the smallest divisor of ``rh`` that is ``>= min(T, rh)``
(``tw`` likewise) and it is tiled when ``nh * nw = (rh / th) * (rw / tw) > 1``.  Tile ``(i, j)`` of a sample holds the tokens
``(i th + y, j tw + x)``, row-major inside the tile, the tiles row-major in the sample.  ``attn1`` of a tiled block attends
inside a tile only -- same weights, heads and scale -- and nothing else in the block changes.

``transformer_block`` restates ``oracle.unet.transformer_block`` with the tile rearrangement around ``attn1``; ``patched(run)``
puts it in place of the one ``oracle.unet``, ``tests.sd2_oracle`` and ``tests.controlnet_oracle`` look up in their modules, for
one forward.  It calls ``oracle.unet._attention`` through the module, so the hooks of ``tests.tgate_oracle`` and
``tests.ip_adapter_oracle`` (which replace that function) compose with it.
"""
from __future__ import annotations

import contextlib

import torch
import torch.nn.functional as F

UNET_TOL = 2e-2                     # tests/test_unet_gpu.py
FLOOR = 5 * UNET_TOL                # what the oracle's own tiled-against-plain distance must exceed at every UNet case


def tile_side(r: int, T: int) -> int:
    """The smallest divisor of ``r`` that is ``>= min(T, r)``."""
    return next(d for d in range(min(T, r), r + 1) if r % d == 0)


def tiling(rh: int, rw: int, T: int):
    """(nh, nw, th, tw) of a block on ``rh x rw`` tokens; ``nh * nw == 1``: one tile, the block is not tiled."""
    th, tw = tile_side(rh, T), tile_side(rw, T)
    return rh // th, rw // tw, th, tw


def gather_index(rh: int, rw: int, nh: int, nw: int) -> torch.Tensor:
    """[rh * rw] int64: the raster token index of every tile-order row of one sample, from the definition (loops)."""
    th, tw = rh // nh, rw // nw
    out = []
    for i in range(nh):
        for j in range(nw):
            for y in range(th):
                for x in range(tw):
                    out.append((i * th + y) * rw + j * tw + x)
    return torch.tensor(out, dtype=torch.long)


def scatter_index(rh: int, rw: int, nh: int, nw: int) -> torch.Tensor:
    """[rh * rw] int64: the tile-order row of every raster token (the inverse permutation of ``gather_index``)."""
    g = gather_index(rh, rw, nh, nw)
    inv = torch.empty_like(g)
    inv[g] = torch.arange(g.numel())
    return inv


def to_tiles(x: torch.Tensor, rh: int, rw: int, nh: int, nw: int) -> torch.Tensor:
    """[B, rh * rw, C] raster rows -> [B * nh * nw, th * tw, C]: every tile a sample of its own."""
    b, n, c = x.shape
    th, tw = rh // nh, rw // nw
    return x.reshape(b, nh, th, nw, tw, c).permute(0, 1, 3, 2, 4, 5).reshape(b * nh * nw, th * tw, c)


def from_tiles(y: torch.Tensor, rh: int, rw: int, nh: int, nw: int) -> torch.Tensor:
    """The inverse of ``to_tiles``."""
    th, tw = rh // nh, rw // nw
    b, c = y.shape[0] // (nh * nw), y.shape[-1]
    return y.reshape(b, nh, nw, th, tw, c).permute(0, 1, 3, 2, 4, 5).reshape(b, rh * rw, c)


class TileRun:
    """The setting of one oracle forward: ``T`` tokens per tile side (0 = off) up to ``max_depth`` on a latent of ``sample_hw``.
    ``used`` collects (rh, rw, nh, nw) of every block that ran tiled, in call order (down, mid, up: the library's plan order)."""

    def __init__(self, sample_hw, T: int, max_depth: int = 0):
        self.sample_hw, self.T, self.max_depth = sample_hw, T, max_depth
        self.used = []

    def tiles(self, hh: int, ww: int):
        if self.T <= 0 or self.sample_hw[0] // hh > 2 ** self.max_depth:
            return 1, 1
        nh, nw, _, _ = tiling(hh, ww, self.T)
        return nh, nw


def tiled_grids(cfg, h: int, w: int, T: int, max_depth: int):
    """(rh, rw, nh, nw) of every tiled block of a ``h x w`` latent in call order, from the config alone."""
    nlev = len(cfg.block_out_channels)
    run = TileRun((h, w), T, max_depth)

    def grid(i):
        rh, rw = h >> i, w >> i
        return (rh, rw) + run.tiles(rh, rw)
    levels = [i for i in range(nlev) if cfg.attn_levels[i] for _ in range(cfg.layers_per_block)] + [nlev - 1] + \
             [i for i in reversed(range(nlev)) if cfg.attn_levels[i] for _ in range(cfg.layers_per_block + 1)]
    return [g for g in map(grid, levels) if g[2] * g[3] > 1]


_ORIG = {}


def transformer_block(w, p: str, x: torch.Tensor, ctx: torch.Tensor, cfg, fq=None, run: TileRun = None) -> torch.Tensor:
    """``oracle.unet.transformer_block`` with ``attn1`` inside the tiles of a tiled block."""
    import oracle.unet as ou
    b, c, hh, ww = x.shape
    nh, nw = run.tiles(hh, ww) if run is not None else (1, 1)
    if nh * nw == 1:
        return _ORIG["unet"](w, p, x, ctx, cfg, fq)
    assert fq is None, "HyperTile on fp8 handles is not built"
    ou._tick()
    run.used.append((hh, ww, nh, nw))
    res = x
    h = F.group_norm(x, cfg.norm_num_groups, w[p + "norm.weight"], w[p + "norm.bias"], 1e-6)
    h = F.conv2d(h, w[p + "proj_in.weight"], w[p + "proj_in.bias"])
    h = h.permute(0, 2, 3, 1).reshape(b, hh * ww, c)
    t = p + "transformer_blocks.0."
    n1 = to_tiles(F.layer_norm(h, (c,), w[t + "norm1.weight"], w[t + "norm1.bias"], 1e-5), hh, ww, nh, nw)
    h = h + from_tiles(ou._attention(w, t + "attn1.", n1, n1, cfg.num_heads), hh, ww, nh, nw)
    n2 = F.layer_norm(h, (c,), w[t + "norm2.weight"], w[t + "norm2.bias"], 1e-5)
    h = h + ou._attention(w, t + "attn2.", n2, ctx, cfg.num_heads)
    n3 = F.layer_norm(h, (c,), w[t + "norm3.weight"], w[t + "norm3.bias"], 1e-5)
    proj = F.linear(n3, w[t + "ff.net.0.proj.weight"], w[t + "ff.net.0.proj.bias"])
    a, gate = proj.chunk(2, dim=-1)
    h = h + F.linear(a * F.gelu(gate), w[t + "ff.net.2.weight"], w[t + "ff.net.2.bias"])
    h = h.reshape(b, hh, ww, c).permute(0, 3, 1, 2)
    h = F.conv2d(h, w[p + "proj_out.weight"], w[p + "proj_out.bias"])
    return h + res


@contextlib.contextmanager
def patched(run: TileRun):
    """For the duration of one forward ``transformer_block`` of ``oracle.unet``, ``tests.sd2_oracle`` and
    ``tests.controlnet_oracle`` is the function above.  (A ControlNet's own forward must run OUTSIDE: it never tiles.)"""
    import oracle.unet as ou
    import tests.controlnet_oracle as co
    import tests.sd2_oracle as s2
    mods = (ou, s2, co)
    origs = [m.transformer_block for m in mods]
    _ORIG["unet"] = ou.transformer_block

    def tb(w, p, x, ctx, cfg, fq=None):
        return transformer_block(w, p, x, ctx, cfg, fq, run)
    for m in mods:
        m.transformer_block = tb
    try:
        yield
    finally:
        for m, o in zip(mods, origs):
            m.transformer_block = o
        _ORIG.pop("unet")


def unet_forward(w, cfg, sample, t, ctx, run: TileRun, heads_per_level=None, **kw):
    """eps of the oracle UNet tiled as ``run`` describes (``heads_per_level``: the SD 2.x-shaped oracle)."""
    with patched(run), torch.no_grad():
        if heads_per_level is not None:
            from tests.sd2_oracle import sd2_unet_forward
            return sd2_unet_forward(w, cfg, heads_per_level, sample, t, ctx, **kw)
        import oracle.unet as ou
        return ou.unet_forward(w, cfg, sample, t, ctx, **kw)


#             env        h   w   lb  ub  seed  t      T   max_depth  tiled blocks
UNET_CASES = [("sd15", 16, 16, 2, 4, 29, 981.0, 8, 0, 5),              # level 0: 2x2 tiles of 64 tokens
              ("sd15", 16, 24, 2, 4, 29, 981.0, 8, 0, 5),              # non-square: 2x3 tiles
              ("sd15", 32, 32, 1, 2, 29, 981.0, 8, 2, 10),             # 4x4 on level 0, 2x2 on level 1; level 2 (8x8 tokens) is one tile
              # 32x32 latents on the 320 / 640 UNet, batch 16 of 8 latents under CFG.  T = 16: level 0 runs 2x2 tiles of 256 keys
              # (the head-major K / V path, attn_pipe40_kernel); T = 8, depth 1: 4x4 tiles of 64 keys on level 0, 2x2 on level 1
              ("two_level", 32, 32, 8, 16, 7, 501.0, 16, 0, 5),
              ("two_level", 32, 32, 8, 16, 7, 501.0, 8, 1, 11)]
SD2_CASE = ("sd2", 16, 16, 1, 2, 29, 981.0, 8, 0, 5)


def unet_inputs(cfg, h: int, w: int, lb: int, ub: int, seed: int = 29):
    """(latents [lb], prompt rows [ub], UNet sample [ub] = the latents repeated): the inputs of the UNet cases, the same for the
    GPU test and for the CPU test that checks the oracle's own tiled-against-plain distance at them first (the draw of
    ``tests.tome_oracle.unet_inputs``, without its choice array)."""
    g = torch.Generator().manual_seed(seed)
    lat = torch.randn(lb, 4, h, w, generator=g)
    ctx = torch.randn(ub, cfg.context_len, cfg.cross_attention_dim, generator=g)
    return lat, ctx, torch.cat([lat] * (ub // lb))


_ENVS, _REF = {}, {}          # per UNet its weights; per case the oracle's forwards: computed once per process, never modified


def env(name: str):
    from tests.tome_oracle import unet_env
    if name not in _ENVS:
        _ENVS[name] = unet_env(name)
    return _ENVS[name]


def reference(case):
    """dict(plain = eps of the plain oracle, tiled = eps of the tiled oracle, used = the tiled blocks in call order) at a case of
    ``UNET_CASES`` / ``SD2_CASE``, cached; the plain forward is shared by the cases that differ in the setting alone."""
    name, h, w, lb, ub, seed, t, T, md, _ = case
    cfg, sd, ocfg, heads = env(name)
    lat, ctx, sample = unet_inputs(cfg, h, w, lb, ub, seed)
    pk = ("plain", name, h, w, lb, ub, seed, t)
    if pk not in _REF:
        _REF[pk] = unet_forward(sd, ocfg, sample, t, ctx, TileRun((h, w), 0), heads_per_level=heads)
    if case not in _REF:
        run = TileRun((h, w), T, md)
        _REF[case] = dict(plain=_REF[pk], tiled=unet_forward(sd, ocfg, sample, t, ctx, run, heads_per_level=heads), used=run.used)
    return _REF[case]
