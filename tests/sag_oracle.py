"""Self-attention guidance (SAG; Hong et al. 2023, diffusers' ``StableDiffusionSAGPipeline``) restated on the torch
oracle: TEST INFRASTRUCTURE (upstream-recall, no upstream text).

Semantics, per step at timestep ``t`` with ``a = alphas_cumprod[t]`` and ``lb`` latents ``x``:

1. forward 1, the normal one: ``[uncond | cond]`` (``ub = 2 lb``) with CFG, ``[cond]`` without.  It also yields the attention
   mass of ``mid_block.attentions.0.transformer_blocks.0.attn1`` for its first ``lb`` samples:
   ``mass[b][k] = (1 / heads) sum_h sum_q softmax_k(Q_h K_h^T / sqrt(d))[q][k]`` -- the masses of a sample average exactly 1.
2. ``m`` = that branch's output (``u`` with CFG, ``c`` without); ``x0`` and ``eps`` from ``(x, m, a)`` by prediction type.
3. ``mask = mass > 1.0`` (strict) on the ``mh x mw`` mid grid, nearest-upsampled by 8 to the latent, the same for all channels.
4. ``blur`` = 9x9 Gaussian of ``x0`` per channel, sigma 1, weights ``exp(-0.5 i^2)`` normalised, reflect padding;
   ``degraded = blur mask + x0 (1 - mask)``; ``x_deg = sqrt(a) degraded + sqrt(1 - a) eps``.
5. forward 2: the UNet at batch ``lb`` on ``x_deg`` at the same ``t`` with the first ``lb`` prompt rows; output ``d``.
6. ``e = (u + g (c - u)) + s (u - d)`` with CFG, ``e = c + s (c - d)`` without; then the scheduler step as ever.

The mask is a threshold at the MEAN of the masses, so some tokens always sit near it: every mask comparison leaves out the tokens
whose oracle mass lies within a band of 1.0 and caps the left-out share; ``reference`` and ``sag_step`` derive the band from the
oracle alone.  ``patched(run)`` puts ``attention`` below in place of ``oracle.unet._attention``, as ``tests.pag_oracle`` does.
"""
from __future__ import annotations

import contextlib
import math

import torch
import torch.nn.functional as F

UNET_TOL = 2e-2                     # tests/test_unet_gpu.py
FREE_TOL, FREE_COS = 6e-2, 0.998    # tests/test_pipeline_gpu.py
MOVED_FLOOR = 0.10                  # one SAG step at s = 0.75 moves the guided prediction by at least this (rel-L2)
SAG_SCALE, GS = 0.75, 7.5
MID_ATTN1 = "mid_block.attentions.0.transformer_blocks.0.attn1."
PRED_IDS = {"epsilon": 0, "v_prediction": 1, "sample": 2}


# ---------------------------------------------------------------------------------------------------------------- the pieces
def attn_mass(q: torch.Tensor, k: torch.Tensor, heads: int, scale: float = None) -> torch.Tensor:
    """mass [B, N] from q, k [B, N, C] (``scale`` None: 1 / sqrt(d); the inputs' dtype is kept -- pass fp64 for a reference)."""
    b, n, c = q.shape
    d = c // heads
    s = (1.0 / math.sqrt(d)) if scale is None else scale
    qh = q.view(b, n, heads, d).transpose(1, 2)
    kh = k.view(b, n, heads, d).transpose(1, 2)
    p = torch.softmax(qh @ kh.transpose(-1, -2) * s, dim=-1)          # [B, heads, Nq, Nk]
    return p.sum(dim=2).mean(dim=1)


def mask_of(mass: torch.Tensor) -> torch.Tensor:
    return mass > 1.0


def upsample8(grid: torch.Tensor) -> torch.Tensor:
    """[B, mh, mw] -> [B, 1, 8 mh, 8 mw], nearest: out[y][x] = grid[y // 8][x // 8]."""
    return grid.repeat_interleave(8, dim=-2).repeat_interleave(8, dim=-1).unsqueeze(1)


def gauss_weights(dtype=torch.float64) -> torch.Tensor:
    w = torch.exp(-0.5 * torch.arange(-4, 5, dtype=torch.float64) ** 2)
    return (w / w.sum()).to(dtype)


def blur(x0: torch.Tensor) -> torch.Tensor:
    """The 9x9 Gaussian (outer product of the 1-D weights) with reflect padding, written out as shifted sums (no conv call)."""
    w = gauss_weights(x0.dtype)
    H, W = x0.shape[-2:]
    p = F.pad(x0, (4, 4, 4, 4), mode="reflect")
    rows = sum(w[i] * p[..., :, i:i + W] for i in range(9))
    return sum(w[i] * rows[..., i:i + H, :] for i in range(9))


def x0_eps(x, m, a: float, pred: str):
    sa, s1 = math.sqrt(a), math.sqrt(1.0 - a)
    if pred == "epsilon":
        return (x - s1 * m) / sa, m
    if pred == "v_prediction":
        return sa * x - s1 * m, sa * m + s1 * x
    if pred == "sample":
        return m, (x - sa * m) / s1
    raise ValueError(pred)


def degrade(x, m, a: float, pred: str, mask_grid: torch.Tensor):
    """x_deg from the latents, the model output on them and the boolean mid-grid mask [B, mh, mw]."""
    x0, eps = x0_eps(x, m, a, pred)
    mk = upsample8(mask_grid).to(x0.dtype)
    deg = blur(x0) * mk + x0 * (1 - mk)
    return math.sqrt(a) * deg + math.sqrt(1.0 - a) * eps


def combine(eps1: torch.Tensor, d: torch.Tensor, lb: int, cfg: bool, g: float, s: float) -> torch.Tensor:
    if cfg:
        u, c = eps1[:lb], eps1[lb:]
        return (u + g * (c - u)) + s * (u - d)
    return eps1 + s * (eps1 - d)


def cfg_step_bound(r, lb: int, g: float = None, s: float = None) -> float:
    """The bound on the rel-L2 error of a CFG SAG step's ``e`` that follows from UNET_TOL per UNet output, from the ORACLE's step
    ``r`` alone (``sag_step`` with its own mask): e = (1 - g + s) u + g c - s d, each of u, c, d within UNET_TOL of its norm, so
    |de| <= UNET_TOL (|1 - g + s| |u| + g |c| + s |d|), over |e|."""
    g, s = GS if g is None else g, SAG_SCALE if s is None else s
    u, c, d = r["eps1"][:lb], r["eps1"][lb:], r["d"]
    return float(UNET_TOL * (abs(1.0 - g + s) * u.norm() + g * c.norm() + s * d.norm()) / r["e"].norm())


def plain_guided(eps1, lb, cfg, g):
    return eps1[:lb] + g * (eps1[lb:] - eps1[:lb]) if cfg else eps1


# ------------------------------------------------------------------------------------------------------- the patched oracle
class SagRun:
    """One oracle forward with capture: ``mass`` [B, N] of the mid block's attn1 (fp32, from the block's own q and k);
    ``noise_rel`` > 0 also computes ``mass_pert`` from the attn1 input (the norm1 output) plus seeded Gaussian noise of that
    rel-L2 -- the forward itself runs on the clean input."""

    def __init__(self, noise_rel: float = 0.0, noise_seed: int = 0):
        self.noise_rel, self.noise_seed = noise_rel, noise_seed
        self.mass = self.mass_pert = None


_ORIG = {}


def attention(w, p, x, ctx, heads, fq=None, run: SagRun = None):
    if run is not None and p == MID_ATTN1:
        assert fq is None, "SAG on fp8 handles is not built"
        run.mass = attn_mass(F.linear(x, w[p + "to_q.weight"]), F.linear(x, w[p + "to_k.weight"]), heads)
        if run.noise_rel > 0.0:
            z = torch.randn(x.shape, generator=torch.Generator().manual_seed(run.noise_seed))
            xp = x + z * (run.noise_rel * x.norm() / z.norm())
            run.mass_pert = attn_mass(F.linear(xp, w[p + "to_q.weight"]), F.linear(xp, w[p + "to_k.weight"]), heads)
    return _ORIG["attention"](w, p, x, ctx, heads, fq)


@contextlib.contextmanager
def patched(run: SagRun):
    import oracle.unet as ou
    _ORIG["attention"] = ou._attention

    def att(w, p, x, ctx, heads, fq=None):
        return attention(w, p, x, ctx, heads, fq, run)
    ou._attention = att
    try:
        yield
    finally:
        ou._attention = _ORIG.pop("attention")


def unet_forward(w, cfg, sample, t, ctx, run: SagRun = None, heads_per_level=None, tile=None):
    """eps of the oracle UNet; with ``run`` the mid block's attention mass is captured (``tile``: a
    ``tests.hypertile_oracle.TileRun``)."""
    import tests.hypertile_oracle as ho
    tile = tile if tile is not None else ho.TileRun(tuple(sample.shape[-2:]), 0)
    if run is None:
        return ho.unet_forward(w, cfg, sample, t, ctx, tile, heads_per_level=heads_per_level)
    with patched(run):
        return ho.unet_forward(w, cfg, sample, t, ctx, tile, heads_per_level=heads_per_level)


@torch.no_grad()
def sag_step(w, ocfg, x, t, a: float, pred: str, ctx, cfg: bool, g: float, s: float, heads_per_level=None, forced_mask=None,
             tile_fn=None):
    """One SAG step's prediction.  ``forced_mask`` [lb, mh, mw] bool replaces the oracle's own mask.  Returns dict(e, eps1, d,
    mass [lb, mh, mw] -- the oracle's own -- and plain = the guided prediction without SAG)."""
    lb = x.shape[0]
    f = 2 ** (len(ocfg.block_out_channels) - 1)
    mh, mw = x.shape[-2] // f, x.shape[-1] // f
    run = SagRun(noise_rel=UNET_TOL, noise_seed=int(t) + 1)
    tile = (lambda: tile_fn()) if tile_fn is not None else (lambda: None)
    eps1 = unet_forward(w, ocfg, torch.cat([x] * (ctx.shape[0] // lb)), t, ctx, run, heads_per_level, tile())
    mass = run.mass[:lb].view(lb, mh, mw)
    grid = mask_of(mass) if forced_mask is None else forced_mask
    xd = degrade(x, eps1[:lb], a, pred, grid)
    # (s = 0, the plain loop of a comparison: d carries no weight, the second forward is not run)
    d = unet_forward(w, ocfg, xd, t, ctx[:lb], None, heads_per_level, tile()) if s != 0.0 else eps1[:lb]
    shift = float((run.mass_pert[:lb] - run.mass[:lb]).abs().max())
    return dict(e=combine(eps1, d, lb, cfg, g, s), eps1=eps1, d=d, mass=mass, plain=plain_guided(eps1, lb, cfg, g), x_deg=xd,
                band=BAND_FACTOR * shift)


@torch.no_grad()
def loop(w, ocfg, step_fn, alphas_cumprod, pred: str, timesteps, pe, ne, lat, g: float, s: float, heads_per_level=None,
         forced_masks=None, tile_fn=None):
    """The sampling loop with SAG.  ``step_fn(e, t, x) -> x``: the scheduler step; ``forced_masks``: one [lb, mh, mw] bool
    tensor per step in place of the oracle's own.  Returns (final latents, the oracle's own masses per step, the band of each
    step: BAND_FACTOR x the shift of that step's mass under noise of rel-L2 UNET_TOL on the attn1 input)."""
    cfg = ne is not None
    ctx = torch.cat([ne, pe]) if cfg else pe
    x = lat.float()
    masses, bands = [], []
    for i, t in enumerate(timesteps):
        r = sag_step(w, ocfg, x, t, float(alphas_cumprod[int(t)]), pred, ctx, cfg, g, s, heads_per_level,
                     None if forced_masks is None else forced_masks[i], tile_fn)
        masses.append(r["mass"])
        bands.append(r["band"])
        x = step_fn(r["e"], t, x).float()
    return x, masses, bands


def masks_agree(own_mass: torch.Tensor, got_mask: torch.Tensor, band: float, cap: float, what: str) -> float:
    """Assert ``got_mask`` equals ``own_mass > 1`` at every token whose oracle mass is at least ``band`` from 1.0, and that at
    most ``cap`` of the tokens are left out.  Returns the left-out share."""
    near = (own_mass - 1.0).abs() <= band
    share = float(near.float().mean())
    bad = int(((mask_of(own_mass) != got_mask) & ~near).sum())
    print(f"[sag mask] {what}: {share:.3f} of the tokens within {band:.4f} of the threshold (cap {cap}), {bad} differ outside it")
    assert share <= cap, f"{what}: {share:.3f} of the tokens lie within the band (cap {cap})"
    assert bad == 0, f"{what}: {bad} mask tokens differ outside the band"
    return share


# ------------------------------------------------------------------------------------------------------------- the cases
#              env          h   w   lb  seed   t
UNET_CASES = [("sd15", 32, 32, 2, 29, 981.0),            # mid grid 4x4: 16 tokens, d = 160
              ("sd15", 32, 40, 1, 29, 501.0),            # 4x5: 20 tokens, no multiple of 16
              ("sd2", 32, 32, 1, 29, 501.0),             # d = 64, 20 heads
              ("two_level", 32, 32, 1, 29, 21.0)]        # 16x16: 256 mid tokens, d = 80
# the full SAG step, per guidance mode, chosen from the oracle's own figures (tests/test_sag_cpu.py asserts them): with CFG 7.5 the
# step moves the guided prediction by 0.166 at t = 981 and by 0.086 < MOVED_FLOOR at t = 501; without CFG 0.344 of the tokens lie
# inside the band at t = 981 (above MASK_CAP) and 0.094 at t = 501, where the step moves 0.191
STEP_CASES = {True: UNET_CASES[0], False: ("sd15", 32, 32, 2, 29, 501.0)}
BAND_FACTOR = 1.5
MASK_CAP = 0.30

_ENVS, _REF = {}, {}          # per UNet its weights; per case the oracle's forwards: computed once per process, never modified


def env(name: str):
    from tests.tome_oracle import unet_env
    if name not in _ENVS:
        _ENVS[name] = unet_env(name)
    return _ENVS[name]


def unet_inputs(cfg, h, w, lb, seed=29):
    g = torch.Generator().manual_seed(seed)
    lat = torch.randn(lb, 4, h, w, generator=g)
    two = torch.randn(2 * lb, cfg.context_len, cfg.cross_attention_dim, generator=g)
    return lat, two[lb:], two[:lb]          # latents, positive rows, negative rows


def reference(case):
    """dict(eps, mass [ub, N], band) of the oracle's CFG forward at a UNet case, cached.  ``band`` = BAND_FACTOR x the largest
    shift of the oracle's own mass when the attn1 input is perturbed by seeded noise of rel-L2 UNET_TOL."""
    if case not in _REF:
        name, h, w, lb, seed, t = case
        cfg, sd, ocfg, heads = env(name)
        lat, pe, ne = unet_inputs(cfg, h, w, lb, seed)
        run = SagRun(noise_rel=UNET_TOL, noise_seed=seed + 1)
        with torch.no_grad():
            eps = unet_forward(sd, ocfg, torch.cat([lat, lat]), t, torch.cat([ne, pe]), run, heads)
        shift = float((run.mass_pert - run.mass).abs().max())
        _REF[case] = dict(eps=eps, mass=run.mass, shift=shift, band=BAND_FACTOR * shift)
    return _REF[case]


def step_reference(case, forced_mask=None, cfg=True):
    """The oracle's full SAG step (epsilon prediction) at a case; cached per (case, cfg) when no mask is forced."""
    key = ("step", case, cfg)
    if forced_mask is None and key in _REF:
        return _REF[key]
    name, h, w, lb, seed, t = case
    c, sd, ocfg, heads = env(name)
    lat, pe, ne = unet_inputs(c, h, w, lb, seed)
    from oracle.schedulers import DDIMOracle
    a = float(DDIMOracle().alphas_cumprod[int(t)])
    ctx = torch.cat([ne, pe]) if cfg else pe
    r = sag_step(sd, ocfg, lat, t, a, "epsilon", ctx, cfg, GS if cfg else 1.0, SAG_SCALE, heads, forced_mask)
    if forced_mask is None:
        _REF[key] = r
    return r
