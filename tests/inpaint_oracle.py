"""fp32 CPU restatement of diffusers' ``StableDiffusionInpaintPipeline`` without ``padding_mask_crop`` (upstream-recall;
TEST INFRASTRUCTURE like ``oracle/``), on ``oracle.unet.unet_forward`` (generic in ``in_channels`` through ``F.conv2d``),
``tests/vae_encoder_oracle.py`` and the ``oracle.schedulers`` classes.

Mask: binarised in pixel space (``m >= 0.5`` -> 1 = repaint), masked image ``(2 img - 1) (m < 0.5)`` -- in the encoder's
[0, 1] input domain ``keep ? img : 0.5`` --, latent mask = nearest resize = the pixel at ``(8 i, 8 j)``.
Draws from ONE generator, in order: posterior noise of the image latents (``sample_mode="sample"``; not when ``latents`` is
given for a 9-channel UNet), forward noise (unless ``latents``), posterior noise of the masked-image latents (9 channels).
Start: ``noise * init_noise_sigma`` at strength 1.0, ``add_noise(image latents, noise, t_0)`` below.
4-channel loop: after every ``scheduler.step``, ``latents = m ? prev : add_noise(image latents, noise, t_{i+1})``, the image
latents themselves after the last step.  9-channel loop: the UNet reads ``cat([latents, mask, masked-image latents], 1)``.
"""
from __future__ import annotations

import torch

from tests.vae_encoder_oracle import add_noise_coefs, posterior_sample, vae_encode


def prepare_mask(image: torch.Tensor, mask: torch.Tensor):
    """(masked image in [0, 1], latent mask [B,1,H/8,W/8] 0 / 1) of image [B,3,H,W] and mask [B,1,H,W]."""
    rep = mask >= 0.5
    return torch.where(rep, torch.full_like(image, 0.5), image), rep[..., ::8, ::8].float()


@torch.no_grad()
def inpaint_loop(unet_w, unet_cfg, vae_w, vae_cfg, sched, prompt_embeds, negative_prompt_embeds, images, mask, n, strength,
                 guidance_scale, generator, sample_mode="sample", lcm_noise=None, deepcache=None, latents=None,
                 guidance_rescale=0.0):
    """Returns (final latents, start latents, steps run, image latents or None, latent mask)."""
    from oracle.unet import unet_forward
    nine = unet_cfg.in_channels == 9
    init_steps = min(int(n * strength), n)
    t_start = max(n - init_steps, 0)
    do_cfg = guidance_scale > 1.0
    ctx = torch.cat([negative_prompt_embeds, prompt_embeds]) if do_cfg else prompt_embeds
    sched.set_timesteps(n)
    timesteps = [int(t) for t in sched.timesteps][t_start:]
    masked_img, lmask = prepare_mask(images, mask)
    b, _, hh, ww = images.shape
    shape = (b, 4, hh // 8, ww // 8)
    init = None
    if not (nine and latents is not None):
        post = torch.randn(shape, generator=generator) if sample_mode == "sample" else None
        init = posterior_sample(vae_encode(vae_w, vae_cfg, images), post, sample_mode, vae_cfg.scaling_factor)
    noise = latents.float() if latents is not None else torch.randn(shape, generator=generator)
    masked_lat = None
    if nine:
        post = torch.randn(shape, generator=generator) if sample_mode == "sample" else None
        masked_lat = posterior_sample(vae_encode(vae_w, vae_cfg, masked_img), post, sample_mode, vae_cfg.scaling_factor)
    if strength == 1.0:
        start = noise * sched.init_noise_sigma
    else:
        alpha, sigma = add_noise_coefs(sched, t_start)
        start = alpha * init + sigma * noise
    x = start.clone()
    if deepcache is not None:
        deepcache.cached.clear()
        deepcache.start_timestep = None
    for i, t in enumerate(timesteps):
        xin = torch.cat([x, lmask, masked_lat], 1) if nine else x
        lin = torch.cat([xin] * 2) if do_cfg else xin
        if deepcache is not None:
            deepcache.cur_timestep = i
        e = unet_forward(unet_w, unet_cfg, lin, torch.tensor(t), ctx, dc=deepcache)
        if do_cfg:
            u, c = e.chunk(2)
            e = u + guidance_scale * (c - u)
            if guidance_rescale > 0.0:
                from tests.sched_ref import rescale_noise_cfg
                e = rescale_noise_cfg(e, c, guidance_rescale).float()
        kw = {}
        if lcm_noise is not None and i < len(timesteps) - 1:
            kw["noise"] = lcm_noise[i]
        x = sched.step(e, t, x, return_dict=False, **kw)[0]
        if not nine:
            if i < len(timesteps) - 1:
                alpha, sigma = add_noise_coefs(sched, t_start + i + 1)
                proper = alpha * init + sigma * noise
            else:
                proper = init
            x = torch.where(lmask >= 0.5, x, proper)
    return x, start, len(timesteps), init, lmask
