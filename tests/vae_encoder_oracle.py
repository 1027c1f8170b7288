"""fp32 CPU restatement of diffusers 0.32.1 ``AutoencoderKL.encode`` for the SD-1.5 VAE and of the start of
``StableDiffusionImg2ImgPipeline`` (upstream-recall; TEST INFRASTRUCTURE like ``oracle/``).

``vae_encode``: ``x = 2 img - 1`` -> encoder.conv_in -> 4 down blocks of 2 ResNets (128, 256, 512, 512; the first three
followed by ``F.pad(x, (0, 1, 0, 1))`` + an UNPADDED stride-2 3x3 conv) -> mid block (ResNet, single-head attention, ResNet)
-> GroupNorm(32, 1e-6) + SiLU -> conv_out (512 -> 8) -> quant_conv (1x1) -> moments ``[mean | logvar]``.
``posterior_sample``: ``DiagonalGaussianDistribution.sample() / .mode()`` times the scaling factor.
``img2img_loop``: encode, posterior draw, forward-noise draw (in that order, from one generator), ``add_noise`` at the first
timestep that runs, then the ``oracle.schedulers`` classes stepped from index ``t_start`` with ``oracle.unet.unet_forward``.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from oracle.vae import _attention, _resnet


def downsample(x, w, b):
    """Downsample2D of the VAE encoder (padding = 0): zero-pad right 1 / bottom 1, then 3x3 stride 2 without padding."""
    return F.conv2d(F.pad(x, (0, 1, 0, 1)), w, b, stride=2)


@torch.no_grad()
def vae_encode(w, cfg, images: torch.Tensor) -> torch.Tensor:
    """images [B,3,H,W] in [0,1] -> moments [B,8,H/8,W/8] (fp32)."""
    g = cfg.norm_num_groups
    h = F.conv2d(2.0 * images.float() - 1.0, w["encoder.conv_in.weight"], w["encoder.conv_in.bias"], padding=1)
    nl = len(cfg.block_out_channels)
    for i in range(nl):
        for j in range(cfg.layers_per_block):
            h = _resnet(w, f"encoder.down_blocks.{i}.resnets.{j}.", h, g)
        if i < nl - 1:
            p = f"encoder.down_blocks.{i}.downsamplers.0.conv."
            h = downsample(h, w[p + "weight"], w[p + "bias"])
    h = _resnet(w, "encoder.mid_block.resnets.0.", h, g)
    h = _attention(w, "encoder.mid_block.attentions.0.", h, g)
    h = _resnet(w, "encoder.mid_block.resnets.1.", h, g)
    h = F.silu(F.group_norm(h, g, w["encoder.conv_norm_out.weight"], w["encoder.conv_norm_out.bias"], 1e-6))
    h = F.conv2d(h, w["encoder.conv_out.weight"], w["encoder.conv_out.bias"], padding=1)
    return F.conv2d(h, w["quant_conv.weight"], w["quant_conv.bias"])


def posterior_sample(moments: torch.Tensor, noise=None, mode: str = "sample", scale: float = 1.0) -> torch.Tensor:
    mean, logvar = moments.chunk(2, dim=1)
    if mode == "argmax":
        return scale * mean
    std = torch.exp(0.5 * logvar.clamp(-30.0, 20.0))
    return scale * (mean + std * noise)


def add_noise_coefs(sched, index: int):
    """(alpha, sigma) of x_t = alpha x0 + sigma noise at schedule index ``index``: DPM-Solver from its own sigma table
    (upstream's add_noise with begin_index), DDIM / LCM from alphas_cumprod[t]."""
    if hasattr(sched, "sigmas") and hasattr(sched, "_sigma_to_alpha_sigma_t"):
        a, s = sched._sigma_to_alpha_sigma_t(sched.sigmas[index].double())
        return float(a), float(s)
    ac = sched.alphas_cumprod[int(sched.timesteps[index])].double()
    return float(ac.sqrt()), float((1.0 - ac).sqrt())


@torch.no_grad()
def img2img_loop(unet_w, unet_cfg, vae_w, vae_cfg, sched, prompt_embeds, negative_prompt_embeds, images, n, strength,
                 guidance_scale, generator, sample_mode="sample", lcm_noise=None, deepcache=None):
    """Returns (final latents, noised start latents, steps run)."""
    from oracle.unet import unet_forward
    init_steps = min(int(n * strength), n)
    t_start = max(n - init_steps, 0)
    do_cfg = guidance_scale > 1.0
    ctx = torch.cat([negative_prompt_embeds, prompt_embeds]) if do_cfg else prompt_embeds
    sched.set_timesteps(n)
    timesteps = [int(t) for t in sched.timesteps][t_start:]
    moments = vae_encode(vae_w, vae_cfg, images)
    shape = (moments.shape[0], moments.shape[1] // 2) + tuple(moments.shape[2:])
    post = torch.randn(shape, generator=generator) if sample_mode == "sample" else None
    init = posterior_sample(moments, post, sample_mode, vae_cfg.scaling_factor)
    noise = torch.randn(shape, generator=generator)
    alpha, sigma = add_noise_coefs(sched, t_start)
    start = alpha * init + sigma * noise
    latents = start.clone()
    if deepcache is not None:
        deepcache.cached.clear()
        deepcache.start_timestep = None
    for i, t in enumerate(timesteps):
        lin = torch.cat([latents] * 2) if do_cfg else latents
        if deepcache is not None:
            deepcache.cur_timestep = i              # the plan indexes the list that RUNS: the first executed step is full
        e = unet_forward(unet_w, unet_cfg, lin, torch.tensor(t), ctx, dc=deepcache)
        if do_cfg:
            u, c = e.chunk(2)
            e = u + guidance_scale * (c - u)
        kw = {}
        if lcm_noise is not None and i < len(timesteps) - 1:
            kw["noise"] = lcm_noise[i]
        latents = sched.step(e, t, latents, return_dict=False, **kw)[0]
    return latents, start, len(timesteps)
