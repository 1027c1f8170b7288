"""fp32 CPU restatement of the Stable Diffusion 2.x forward for the parity tests, built from the project's SD-1.5 oracle.

What differs from SD-1.5 (diffusers ``UNet2DConditionModel`` with ``attention_head_dim=[5, 10, 20, 20]``,
``use_linear_projection=True``, ``cross_attention_dim=1024``):

* the head COUNT is a property of the resolution level (the mid block uses the last level's, the up blocks mirror the down
  blocks): ``sd2_unet_forward`` walks the blocks exactly as ``oracle.unet.unet_forward`` does -- the same ``resnet_block``,
  ``transformer_block``, ``timestep_embedding`` and DeepCache wrapper -- and hands ``transformer_block`` a config whose
  ``num_heads`` is the level's;
* ``proj_in`` / ``proj_out`` are Linear layers: per token the same map as the 1x1 conv, so their [C, C] weights are viewed as
  [C, C, 1, 1] (``conv_view``);
* the text tower (OpenCLIP ViT-H) has an exact-gelu MLP: ``clip_text_forward_act``.

``upcast_attention`` needs no restatement: the oracle is fp32 throughout.
"""
from __future__ import annotations

import dataclasses
from typing import Dict, Optional, Sequence

import torch
import torch.nn.functional as F

from oracle.unet import DeepCacheState, UNetConfig, _cached, resnet_block, timestep_embedding, transformer_block


def conv_view(w: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """The state dict with every 2-D transformer ``proj_in`` / ``proj_out`` weight viewed as a 1x1 conv's."""
    return {k: (v[:, :, None, None] if v.dim() == 2 and ".attentions." in k and k.endswith((".proj_in.weight", ".proj_out.weight"))
                else v) for k, v in w.items()}


def oracle_config(cfg) -> UNetConfig:
    """``oracle.unet.UNetConfig`` of a product config (its dataclass fields; the head counts travel separately)."""
    return UNetConfig(**dataclasses.asdict(cfg))


@torch.no_grad()
def sd2_unet_forward(w: Dict[str, torch.Tensor], cfg: UNetConfig, heads: Sequence[int], sample: torch.Tensor, t, ctx: torch.Tensor,
                     dc: Optional[DeepCacheState] = None, taps: Optional[dict] = None, fq=None,
                     down_residuals=None, mid_residual=None) -> torch.Tensor:
    """``oracle.unet.unet_forward`` with ``heads[level]`` heads in the transformer blocks of a level.  ``w`` may hold Linear
    projections.  ``down_residuals`` / ``mid_residual``: ControlNet residuals added to the skip tensors and the mid output."""
    w = conv_view(w)
    n = sample.shape[0]
    nlev = len(cfg.block_out_channels)
    assert len(heads) == nlev
    lcfg = [dataclasses.replace(cfg, num_heads=int(h)) for h in heads]
    tt = torch.as_tensor(t, dtype=torch.float32).reshape(-1)
    if tt.numel() == 1:
        tt = tt.expand(n)
    temb = timestep_embedding(tt, cfg.block_out_channels[0]).to(sample.dtype)
    temb = F.linear(temb, w["time_embedding.linear_1.weight"], w["time_embedding.linear_1.bias"])
    temb = F.silu(temb)
    temb = F.linear(temb, w["time_embedding.linear_2.weight"], w["time_embedding.linear_2.bias"])

    h = F.conv2d(sample, w["conv_in.weight"], w["conv_in.bias"], padding=1)
    if taps is not None:
        taps["conv_in"] = h
    skips = [h]
    for i in range(nlev):
        def run_down(i=i, h_in=h):
            hcur, outs = h_in, []
            for j in range(cfg.layers_per_block):
                p = f"down_blocks.{i}.resnets.{j}."
                hcur = _cached(dc, ("down", "resnet", i, j), i, j, "down",
                               lambda hcur=hcur, p=p: resnet_block(w, p, hcur, temb, cfg, fq))
                if cfg.attn_levels[i]:
                    p = f"down_blocks.{i}.attentions.{j}."
                    hcur = _cached(dc, ("down", "attentions", i, j), i, j, "down",
                                   lambda hcur=hcur, p=p: transformer_block(w, p, hcur, ctx, lcfg[i], fq))
                outs.append(hcur)
            if i < nlev - 1:
                p = f"down_blocks.{i}.downsamplers.0.conv."
                hcur = _cached(dc, ("down", "downsampler", i, cfg.layers_per_block), i, cfg.layers_per_block, "down",
                               lambda hcur=hcur, p=p: F.conv2d(hcur, w[p + "weight"], w[p + "bias"], stride=2, padding=1))
                outs.append(hcur)
            return hcur, outs
        h, outs = _cached(dc, ("down", "block", i, 0), i, 0, "down", run_down)
        skips.extend(outs)
        if taps is not None:
            taps[f"down{i}"] = h

    def run_mid(h_in=h):
        hcur = resnet_block(w, "mid_block.resnets.0.", h_in, temb, cfg, fq)
        hcur = transformer_block(w, "mid_block.attentions.0.", hcur, ctx, lcfg[nlev - 1], fq)
        return resnet_block(w, "mid_block.resnets.1.", hcur, temb, cfg, fq)
    h = _cached(dc, ("mid", "mid_block", 0, 0), 0, 0, "mid", run_mid)
    if taps is not None:
        taps["mid"] = h
    if down_residuals is not None:
        assert len(down_residuals) == len(skips)
        skips = [s + r for s, r in zip(skips, down_residuals)]
        h = h + mid_residual

    nres = cfg.layers_per_block + 1
    for i in range(nlev):
        lev = nlev - 1 - i
        res_samples = skips[-nres:]
        skips = skips[:-nres]
        rb = nlev - 1 - i

        def run_up(i=i, h_in=h, res_samples=res_samples, lev=lev, rb=rb):
            hcur = h_in
            rs = list(res_samples)
            for j in range(nres):
                skip = rs.pop()
                rl = nres - 1 - j
                p = f"up_blocks.{i}.resnets.{j}."
                hcur = _cached(dc, ("up", "resnet", rb, rl), rb, rl, "up",
                               lambda hcur=hcur, skip=skip, p=p: resnet_block(w, p, torch.cat([hcur, skip], dim=1), temb, cfg, fq))
                if cfg.attn_levels[lev]:
                    p = f"up_blocks.{i}.attentions.{j}."
                    hcur = _cached(dc, ("up", "attentions", rb, rl), rb, rl, "up",
                                   lambda hcur=hcur, p=p: transformer_block(w, p, hcur, ctx, lcfg[lev], fq))
            if i < nlev - 1:
                p = f"up_blocks.{i}.upsamplers.0.conv."
                hcur = _cached(dc, ("up", "upsampler", rb, 0), rb, 0, "up",
                               lambda hcur=hcur, p=p: F.conv2d(F.interpolate(hcur, scale_factor=2.0, mode="nearest"),
                                                              w[p + "weight"], w[p + "bias"], padding=1))
            return hcur
        h = _cached(dc, ("up", "block", rb, 0), rb, 0, "up", run_up)
        if taps is not None:
            taps[f"up{i}"] = h

    h = F.group_norm(h, cfg.norm_num_groups, w["conv_norm_out.weight"], w["conv_norm_out.bias"], cfg.norm_eps)
    return F.conv2d(F.silu(h), w["conv_out.weight"], w["conv_out.bias"], padding=1)


@torch.no_grad()
def clip_text_forward_act(w, cfg, input_ids: torch.Tensor, hidden_act: str = "gelu") -> torch.Tensor:
    """``oracle.clip.clip_text_forward`` with the MLP activation as a parameter: ``"gelu"`` is the exact (erf) GELU of the
    OpenCLIP text tower, ``"quick_gelu"`` reproduces the SD-1.5 oracle."""
    act = {"gelu": F.gelu, "quick_gelu": lambda x: x * torch.sigmoid(1.702 * x)}[hidden_act]
    B, L = input_ids.shape
    H, nh = cfg.hidden_size, cfg.num_attention_heads
    d = H // nh
    P = lambda n: w["text_model." + n].float()
    h = P("embeddings.token_embedding.weight")[input_ids.long()] + P("embeddings.position_embedding.weight")[:L]
    mask = torch.full((L, L), float("-inf")).triu(1)
    sp = lambda x: x.view(B, L, nh, d).transpose(1, 2)
    for i in range(cfg.num_hidden_layers):
        p = f"encoder.layers.{i}."
        x = F.layer_norm(h, (H,), P(p + "layer_norm1.weight"), P(p + "layer_norm1.bias"), cfg.layer_norm_eps)
        q = F.linear(x, P(p + "self_attn.q_proj.weight"), P(p + "self_attn.q_proj.bias")) * d ** -0.5
        k = F.linear(x, P(p + "self_attn.k_proj.weight"), P(p + "self_attn.k_proj.bias"))
        v = F.linear(x, P(p + "self_attn.v_proj.weight"), P(p + "self_attn.v_proj.bias"))
        a = (torch.softmax(sp(q) @ sp(k).transpose(-1, -2) + mask, dim=-1) @ sp(v)).transpose(1, 2).reshape(B, L, H)
        h = h + F.linear(a, P(p + "self_attn.out_proj.weight"), P(p + "self_attn.out_proj.bias"))
        x = F.layer_norm(h, (H,), P(p + "layer_norm2.weight"), P(p + "layer_norm2.bias"), cfg.layer_norm_eps)
        h = h + F.linear(act(F.linear(x, P(p + "mlp.fc1.weight"), P(p + "mlp.fc1.bias"))), P(p + "mlp.fc2.weight"), P(p + "mlp.fc2.bias"))
    return F.layer_norm(h, (H,), P("final_layer_norm.weight"), P("final_layer_norm.bias"), cfg.layer_norm_eps)


@torch.no_grad()
def sd2_controlnet_forward(cw, cfg: UNetConfig, heads, sample, t, ctx, cond, conditioning_scale: float = 1.0):
    """``tests.controlnet_oracle.controlnet_forward`` with per-level head counts (and Linear projections in ``cw``): the
    twelve down residuals and the mid residual, NCHW fp32."""
    from tests.controlnet_oracle import _temb, cond_embedding
    cw = conv_view(cw)
    nlev = len(cfg.block_out_channels)
    lcfg = [dataclasses.replace(cfg, num_heads=int(h)) for h in heads]
    temb = _temb(cw, cfg, sample.shape[0], t, sample.dtype)
    emb = cond_embedding(cw, cond)
    if emb.shape[0] != sample.shape[0]:
        emb = emb.repeat(sample.shape[0] // emb.shape[0], 1, 1, 1)
    h = F.conv2d(sample, cw["conv_in.weight"], cw["conv_in.bias"], padding=1) + emb
    skips = [h]
    for i in range(nlev):
        for j in range(cfg.layers_per_block):
            h = resnet_block(cw, f"down_blocks.{i}.resnets.{j}.", h, temb, cfg)
            if cfg.attn_levels[i]:
                h = transformer_block(cw, f"down_blocks.{i}.attentions.{j}.", h, ctx, lcfg[i])
            skips.append(h)
        if i < nlev - 1:
            p = f"down_blocks.{i}.downsamplers.0.conv."
            h = F.conv2d(h, cw[p + "weight"], cw[p + "bias"], stride=2, padding=1)
            skips.append(h)
    h = resnet_block(cw, "mid_block.resnets.0.", h, temb, cfg)
    h = transformer_block(cw, "mid_block.attentions.0.", h, ctx, lcfg[nlev - 1])
    h = resnet_block(cw, "mid_block.resnets.1.", h, temb, cfg)
    down = [F.conv2d(s, cw[f"controlnet_down_blocks.{i}.weight"], cw[f"controlnet_down_blocks.{i}.bias"]) * conditioning_scale
            for i, s in enumerate(skips)]
    return down, F.conv2d(h, cw["controlnet_mid_block.weight"], cw["controlnet_mid_block.bias"]) * conditioning_scale


def gelu_clip_state_dict():
    """(config kwargs, weights) of the tiny gelu text tower of tests/golden/clip_gelu_golden.json: ``CLIP_TINY`` and
    ``make_synthetic_clip_state_dict(seed=777)`` with every ``mlp.fc1.bias`` lowered by 2 and every ``mlp.fc2.weight`` times 4.
    With the plain weights gelu and quick_gelu towers differ by 8.9e-3 rel-L2 (the two functions differ by ~1 % over N(0, 1)
    pre-activations, and the attention branch and the final LayerNorm dilute it): less than the bf16 tolerance of the GPU
    tests, so a tower run with the wrong activation would pass.  The two functions differ most, relatively, in the negative
    tail (gelu(-2.5) = -0.0155, quick_gelu(-2.5) = -0.0350); pre-activations centred there and an MLP branch that carries most
    of the residual stream separate the two fp32 towers by 9.6e-2."""
    from sonicdiffusionbayeslab_amd.clip import ClipTextConfig, make_synthetic_clip_state_dict
    from tests.util import CLIP_TINY
    sd = make_synthetic_clip_state_dict(ClipTextConfig(**CLIP_TINY), seed=777)
    out = {}
    for k, v in sd.items():
        if k.endswith("mlp.fc1.bias"):
            v = (v - 2.0).to(torch.bfloat16).float()
        elif k.endswith("mlp.fc2.weight"):
            v = v * 4.0
        out[k] = v
    return dict(CLIP_TINY), out


@torch.no_grad()
def cfg_loop(w, cfg: UNetConfig, heads, pe, ne, lat, plan, guidance_scale: float, guidance_rescale: float = 0.0):
    """The short classifier-free-guidance loop the pipeline tests need.  ``plan``: [(scheduler restatement of
    tests/sched_ref.py, t)]; the model output is combined (and rescaled) by ``tests.sched_ref.guided``."""
    from tests import sched_ref as R
    ctx = torch.cat([ne, pe])
    x = lat.double()
    for sched, t in plan:
        xin = x.float()
        m = R.guided(sd2_unet_forward(w, cfg, heads, torch.cat([xin, xin]), t, ctx), guidance_scale, guidance_rescale)
        x = sched.step(m, t, x)[0]
    return x
