"""ControlNet oracle for the parity tests: diffusers' ``ControlNetModel.forward`` (``guess_mode=False``) and the residual
injection of ``UNet2DConditionModel.forward`` restated over the CPU oracle's blocks (oracle/unet.py: ``resnet_block``,
``transformer_block``, ``timestep_embedding``), in fp32 on the bf16-grid weights.  upstream-recall; DESIGN.md 4j.

    temb = time_embedding(t)                                          (the ControlNet's own)
    h    = conv_in(sample) + controlnet_cond_embedding(cond)          (cond [N,3,8h,8w] in [0,1], rgb, not normalised)
    the twelve down-block outputs and the mid block exactly as in the UNet, same parameter names
    res_i = controlnet_down_blocks.i(skip_i) (1x1, bias), res_mid = controlnet_mid_block(mid); all times conditioning_scale

UNet side: ``down_block_res_samples[i] += res_i`` AFTER the whole down path (the down path and the mid block see the
unmodified tensors), ``mid += res_mid`` after the mid block."""
import contextlib

import torch
import torch.nn.functional as F

from oracle.unet import resnet_block, timestep_embedding, transformer_block


def _temb(w, cfg, n, t, dtype, timestep_cond=None):
    tt = torch.as_tensor(t, dtype=torch.float32).reshape(-1)
    if tt.numel() == 1:
        tt = tt.expand(n)
    temb = timestep_embedding(tt, cfg.block_out_channels[0]).to(dtype)
    if timestep_cond is not None:        # TimestepEmbedding: sample + cond_proj(condition) before linear_1
        temb = temb + F.linear(timestep_cond.reshape(1, -1).to(dtype), w["time_embedding.cond_proj.weight"])
    temb = F.linear(temb, w["time_embedding.linear_1.weight"], w["time_embedding.linear_1.bias"])
    temb = F.silu(temb)
    return F.linear(temb, w["time_embedding.linear_2.weight"], w["time_embedding.linear_2.bias"])


def _encoder(w, cfg, h, temb, ctx):
    """conv_in's output ``h`` -> (the twelve skips, the mid block's output), in oracle.unet.unet_forward's order of operations."""
    nlev = len(cfg.block_out_channels)
    skips = [h]
    for i in range(nlev):
        for j in range(cfg.layers_per_block):
            h = resnet_block(w, f"down_blocks.{i}.resnets.{j}.", h, temb, cfg)
            if cfg.attn_levels[i]:
                h = transformer_block(w, f"down_blocks.{i}.attentions.{j}.", h, ctx, cfg)
            skips.append(h)
        if i < nlev - 1:
            p = f"down_blocks.{i}.downsamplers.0.conv."
            h = F.conv2d(h, w[p + "weight"], w[p + "bias"], stride=2, padding=1)
            skips.append(h)
    h = resnet_block(w, "mid_block.resnets.0.", h, temb, cfg)
    h = transformer_block(w, "mid_block.attentions.0.", h, ctx, cfg)
    h = resnet_block(w, "mid_block.resnets.1.", h, temb, cfg)
    return skips, h


def cond_embedding(w, cond, round_bf16=False):
    """ControlNetConditioningEmbedding: conv_in, blocks.0..5 (odd ones stride 2), each followed by SiLU, then conv_out.
    ``round_bf16``: round the input and every conv's output to bf16 (where the HIP chain stores a tensor)."""
    r = (lambda x: x.to(torch.bfloat16).float()) if round_bf16 else (lambda x: x)
    p = "controlnet_cond_embedding."
    h = r(F.silu(F.conv2d(r(cond), w[p + "conv_in.weight"], w[p + "conv_in.bias"], padding=1)))
    for i in range(6):
        h = r(F.silu(F.conv2d(h, w[p + f"blocks.{i}.weight"], w[p + f"blocks.{i}.bias"], padding=1, stride=1 + i % 2)))
    return r(F.conv2d(h, w[p + "conv_out.weight"], w[p + "conv_out.bias"], padding=1))


def controlnet_forward(w, cfg, sample, t, ctx, cond, conditioning_scale=1.0, timestep_cond=None):
    """-> (list of the twelve down residuals, the mid residual), NCHW fp32, each times ``conditioning_scale``.
    ``timestep_cond`` [d]: the condition of a ControlNet whose time embedding has a ``cond_proj``."""
    temb = _temb(w, cfg, sample.shape[0], t, sample.dtype, timestep_cond)
    emb = cond_embedding(w, cond)
    if emb.shape[0] != sample.shape[0]:
        emb = emb.repeat(sample.shape[0] // emb.shape[0], 1, 1, 1)
    h = F.conv2d(sample, w["conv_in.weight"], w["conv_in.bias"], padding=1) + emb
    skips, mid = _encoder(w, cfg, h, temb, ctx)
    down = [F.conv2d(s, w[f"controlnet_down_blocks.{i}.weight"], w[f"controlnet_down_blocks.{i}.bias"]) * conditioning_scale
            for i, s in enumerate(skips)]
    return down, F.conv2d(mid, w["controlnet_mid_block.weight"], w["controlnet_mid_block.bias"]) * conditioning_scale


def unet_forward_with_residuals(w, cfg, sample, t, ctx, down_residuals=None, mid_residual=None):
    """oracle.unet.unet_forward with ``down_block_additional_residuals`` / ``mid_block_additional_residual``; with both None
    (or all zeros) it performs unet_forward's operations in unet_forward's order."""
    nlev = len(cfg.block_out_channels)
    temb = _temb(w, cfg, sample.shape[0], t, sample.dtype)
    h = F.conv2d(sample, w["conv_in.weight"], w["conv_in.bias"], padding=1)
    skips, h = _encoder(w, cfg, h, temb, ctx)
    if down_residuals is not None:
        assert len(down_residuals) == len(skips)
        skips = [s + r for s, r in zip(skips, down_residuals)]
    if mid_residual is not None:
        h = h + mid_residual
    nres = cfg.layers_per_block + 1
    for i in range(nlev):
        lev = nlev - 1 - i
        rs, skips = skips[-nres:], skips[:-nres]
        for j in range(nres):
            h = resnet_block(w, f"up_blocks.{i}.resnets.{j}.", torch.cat([h, rs.pop()], dim=1), temb, cfg)
            if cfg.attn_levels[lev]:
                h = transformer_block(w, f"up_blocks.{i}.attentions.{j}.", h, ctx, cfg)
        if i < nlev - 1:
            p = f"up_blocks.{i}.upsamplers.0.conv."
            h = F.conv2d(F.interpolate(h, scale_factor=2.0, mode="nearest"), w[p + "weight"], w[p + "bias"], padding=1)
    h = F.silu(F.group_norm(h, cfg.norm_num_groups, w["conv_norm_out.weight"], w["conv_norm_out.bias"], cfg.norm_eps))
    return F.conv2d(h, w["conv_out.weight"], w["conv_out.bias"], padding=1)


def controlled_unet_forward(w, cw, cfg, sample, t, ctx, cond, scale, unet_ctx=contextlib.nullcontext):
    """eps of the UNet ``w`` conditioned by the ControlNet ``cw`` at ``scale``; scale 0 is the plain forward.  ``unet_ctx()``:
    a context the UNET's forward runs in and the ControlNet's does not (tests/ip_adapter_oracle.py: the ControlNet has no
    image branch)."""
    down = mid = None
    if scale != 0:
        down, mid = controlnet_forward(cw, cfg, sample, t, ctx, cond, scale)
    with unet_ctx():
        return unet_forward_with_residuals(w, cfg, sample, t, ctx, down, mid)


@torch.no_grad()
def control_loop(w, cw, cfg, sched, pos, neg, latents, steps, guidance, cond, scale=1.0, start=0.0, end=1.0,
                 unet_ctx=contextlib.nullcontext):
    """Text-to-image with CFG as oracle.pipeline.sample_loop runs it, every step's UNet conditioned by the ControlNet at
    ``scale * keep_i`` (both CFG halves see the control image).  Returns the final latents."""
    from sonicdiffusionbayeslab_amd.weights import control_keep
    sched.set_timesteps(steps)
    timesteps = sched.timesteps
    keep = control_keep(len(timesteps), start, end)
    x = latents.float() * sched.init_noise_sigma
    ctx = torch.cat([neg, pos])
    for i, t in enumerate(timesteps):
        xin = sched.scale_model_input(torch.cat([x] * 2), t)
        eps = controlled_unet_forward(w, cw, cfg, xin, t, ctx, cond, scale * keep[i], unet_ctx)
        u, c = eps.chunk(2)
        x = sched.step(u + guidance * (c - u), t, x, return_dict=False)[0]
    return x


@contextlib.contextmanager
def controlnet_oracle(cw, cond, scales):
    """Within the block the i-th call of ``oracle.unet.unet_forward`` (looked up at call time: the loop of
    tests/vae_encoder_oracle.py) is conditioned by the ControlNet ``cw`` at ``scales[i]``."""
    import oracle.unet as ounet
    plain, calls = ounet.unet_forward, [0]

    def unet_forward(w, cfg, sample, t, ctx, dc=None, taps=None, fq=None):
        assert dc is None and fq is None, "the ControlNet oracle runs without DeepCache and fp8"
        i = calls[0]
        calls[0] += 1
        return controlled_unet_forward(w, cw, cfg, sample, t, ctx, cond, scales[i])

    ounet.unet_forward = unet_forward
    try:
        yield calls
    finally:
        ounet.unet_forward = plain
