"""FreeU (diffusers ``apply_freeu`` / ``fourier_filter``) restated in torch: TEST INFRASTRUCTURE.

Semantics.  In up block ``i`` in {0, 1}, before each of its three resnets concatenates ``[hidden | skip]``:
``hidden[:, :C_hidden // 2] *= b`` and ``skip = fourier_filter(skip, threshold=1, scale=s)`` with ``(b, s) = (b1, s1)`` for block
0 and ``(b2, s2)`` for block 1.  ``fourier_filter`` per (sample, channel) plane: fftn, fftshift, the box
``[H//2 - 1, H//2 + 1) x [W//2 - 1, W//2 + 1)`` times ``s``, ifftshift, ifftn, real part.  After the shift the box holds the
frequencies {-1, 0} x {-1, 0}, so the filter has the closed form of ``fourier_filter_closed``.

``patched(factors)`` replaces ``resnet_block`` in ``oracle.unet`` and ``tests.sd2_oracle`` for the duration of a forward: the
resnets of up blocks 0 and 1 split their concatenated input at the hidden channel count, apply FreeU without mutating, and call
the original.  Because the hook sits inside the resnet, a DeepCache skip step applies it to the cached feature on consumption.
"""
from __future__ import annotations

import contextlib
import math

import torch

PRESET_SD1 = (0.9, 0.2, 1.5, 1.6)          # the published (s1, s2, b1, b2) for SD 1.x
PLANES = [(2, 2), (4, 4), (5, 7), (8, 12), (9, 18), (16, 16), (32, 32)]
UNET_TOL = 2e-2                             # tests/test_unet_gpu.py


def fourier_filter(x: torch.Tensor, threshold: int = 1, scale: float = 1.0) -> torch.Tensor:
    """diffusers ``fourier_filter`` on [B, C, H, W]; complex arithmetic at the precision of ``x`` (fp32 or fp64)."""
    B, C, H, W = x.shape
    f = torch.fft.fftshift(torch.fft.fftn(x, dim=(-2, -1)), dim=(-2, -1))
    mask = torch.ones((B, C, H, W), dtype=x.dtype)
    cr, cc = H // 2, W // 2
    mask[..., cr - threshold:cr + threshold, cc - threshold:cc + threshold] = scale
    f = f * mask
    return torch.fft.ifftn(torch.fft.ifftshift(f, dim=(-2, -1)), dim=(-2, -1)).real


def fourier_filter_closed(x: torch.Tensor, scale: float) -> torch.Tensor:
    """The same for threshold 1 as seven sums per plane, in fp64:
    y[n] = x[n] + (s - 1) / (H W) (S0 + sum_k C_k cos a_k(n) + S_k sin a_k(n)),  k in {(1,0), (0,1), (1,1)}."""
    xd = x.double()
    H, W = x.shape[-2:]
    a1 = (2.0 * math.pi / H) * torch.arange(H, dtype=torch.float64)[:, None].expand(H, W)
    a2 = (2.0 * math.pi / W) * torch.arange(W, dtype=torch.float64)[None, :].expand(H, W)
    corr = xd.sum(dim=(-2, -1), keepdim=True).expand_as(xd).clone()
    for a in (a1, a2, a1 + a2):
        c, s = torch.cos(a), torch.sin(a)
        corr += (xd * c).sum(dim=(-2, -1), keepdim=True) * c + (xd * s).sum(dim=(-2, -1), keepdim=True) * s
    return xd + (float(scale) - 1.0) / (H * W) * corr


def apply_freeu(block: int, hidden: torch.Tensor, skip: torch.Tensor, s1, s2, b1, b2):
    """diffusers ``apply_freeu`` on NCHW tensors, without mutating its inputs: (hidden', skip')."""
    if block not in (0, 1):
        return hidden, skip
    b, s = (b1, s1) if block == 0 else (b2, s2)
    half = hidden.shape[1] // 2
    hidden = torch.cat([hidden[:, :half] * b, hidden[:, half:]], dim=1)
    return hidden, fourier_filter(skip.float(), 1, s).to(skip.dtype)


def hidden_channels(w, p: str) -> int:
    """Channels of the hidden half of the input of up resnet ``p`` = "up_blocks.<i>.resnets.<j>.": what the previous module
    of the decoder wrote."""
    parts = p.split(".")
    i, j = int(parts[1]), int(parts[3])
    if j > 0:
        prev = f"up_blocks.{i}.resnets.{j - 1}."
    elif i == 0:
        prev = "mid_block.resnets.1."
    else:
        n = max(int(k.split(".")[3]) for k in w if k.startswith(f"up_blocks.{i - 1}.resnets.") and k.endswith("conv2.weight"))
        prev = f"up_blocks.{i - 1}.resnets.{n}."
    return int(w[prev + "conv2.weight"].shape[0])


@contextlib.contextmanager
def patched(factors, calls=None):
    """``factors`` = (s1, s2, b1, b2) or None (off: nothing is patched).  ``calls`` (a list) receives the prefix of every resnet
    FreeU was applied to."""
    if factors is None:
        yield
        return
    import oracle.unet as ou
    import tests.controlnet_oracle as co          # (its UNet with residuals; a ControlNet has no up blocks: its resnets pass through)
    import tests.sd2_oracle as s2
    mods = (ou, s2, co)
    origs = [m.resnet_block for m in mods]
    orig = ou.resnet_block
    f = tuple(float(torch.tensor(v, dtype=torch.float32)) for v in factors)        # the library takes fp32 factors

    def rb(w, p, x, temb, cfg, fq=None):
        if p.startswith("up_blocks.0.") or p.startswith("up_blocks.1."):
            ch = hidden_channels(w, p)
            assert 0 < ch < x.shape[1]
            hidden, skip = apply_freeu(int(p.split(".")[1]), x[:, :ch], x[:, ch:], *f)
            if calls is not None:
                calls.append(p)
            x = torch.cat([hidden, skip], dim=1)
        return orig(w, p, x, temb, cfg, fq)
    for m in mods:
        m.resnet_block = rb
    try:
        yield
    finally:
        for m, o in zip(mods, origs):
            m.resnet_block = o


def unet_forward(w, cfg, sample, t, ctx, factors, heads_per_level=None, calls=None, **kw):
    """eps of the oracle UNet with FreeU at ``factors`` (None: the plain oracle); ``heads_per_level``: the SD 2.x-shaped oracle."""
    with patched(factors, calls), torch.no_grad():
        if heads_per_level is not None:
            from tests.sd2_oracle import sd2_unet_forward
            return sd2_unet_forward(w, cfg, heads_per_level, sample, t, ctx, **kw)
        import oracle.unet as ou
        return ou.unet_forward(w, cfg, sample, t, ctx, **kw)


def unet_inputs(cfg, h: int, w: int, lb: int, ub: int, seed: int = 29):
    """(latents [lb], prompt rows [ub], UNet sample [ub] = the latents repeated): the inputs of the UNet cases, the same for the
    GPU test and for the CPU test that checks the oracle's own with / without distance at them first."""
    g = torch.Generator().manual_seed(seed)
    lat = torch.randn(lb, 4, h, w, generator=g)
    ctx = torch.randn(ub, cfg.context_len, cfg.cross_attention_dim, generator=g)
    return lat, ctx, torch.cat([lat] * (ub // lb))


GIVEN = (0.9, 0.2, 1.2, 1.4)
SWAPPED = (0.2, 0.9, 1.4, 1.2)             # GIVEN with the two blocks' factors exchanged
SINGLE = {"b1": (1.0, 1.0, 1.4, 1.0), "b2": (1.0, 1.0, 1.0, 1.4), "s1": (0.2, 1.0, 1.0, 1.0), "s2": (1.0, 0.2, 1.0, 1.0)}
T_STEP = 981.0

#             id               env          h   w  lb ub factors           floor (x UNET_TOL)
UNET_CASES = [("sd15-16x16-b2", "sd15", 16, 16, 2, 2, GIVEN, 10), ("sd15-16x16-b2_4", "sd15", 16, 16, 2, 4, GIVEN, 10),
              ("sd15-16x24", "sd15", 16, 24, 2, 2, GIVEN, 10), ("sd15-40x40", "sd15", 40, 40, 2, 2, GIVEN, 10),
              ("sd15-b1", "sd15", 16, 16, 2, 2, SINGLE["b1"], 5), ("sd15-b2", "sd15", 16, 16, 2, 2, SINGLE["b2"], 5),
              ("sd15-s1", "sd15", 16, 16, 2, 2, SINGLE["s1"], 5), ("sd15-s2", "sd15", 16, 16, 2, 2, SINGLE["s2"], 5),
              ("sd2-16x16", "sd2", 16, 16, 2, 2, GIVEN, 10), ("two_level-32x32", "two_level", 32, 32, 2, 2, GIVEN, 10)]

_ENVS, _REF = {}, {}          # per UNet its weights; per (UNet, shape, batch, factors) the oracle forward: computed once per process


def env(name: str):
    from tests.tome_oracle import unet_env
    if name not in _ENVS:
        _ENVS[name] = unet_env(name)
    return _ENVS[name]


def reference(name: str, h: int, w: int, lb: int, ub: int, factors, seed: int = 29, t: float = T_STEP):
    """The oracle's eps for a case (``factors`` None: plain), cached and never modified."""
    key = (name, h, w, lb, ub, factors, seed, t)
    if key not in _REF:
        cfg, sd, ocfg, heads = env(name)
        _, ctx, sample = unet_inputs(cfg, h, w, lb, ub, seed)
        _REF[key] = unet_forward(sd, ocfg, sample, t, ctx, factors, heads_per_level=heads)
    return _REF[key]
