"""UNet configuration, parameter enumeration and the synthetic-weight generator.

No SD-1.5 weights exist offline, so benchmarks and parity tests run on
SD-1.5-SHAPED weights drawn from a fixed seed; a local diffusers ``unet`` directory can be
loaded instead when a box has one (``load_unet_state_dict``).  Names and layouts are those of
diffusers' ``UNet2DConditionModel.state_dict()`` -- the same names libsdhip enumerates through
``sd_unet_param_info`` (checked by tests/test_host_cpu.py).
"""
from __future__ import annotations

import math
import os
from dataclasses import InitVar, dataclass
from typing import Dict, List, Optional, Tuple

import torch


@dataclass
class UNetConfig:
    """SD-1.5 UNet2DConditionModel config subset."""
    sample_size: int = 64
    in_channels: int = 4
    out_channels: int = 4
    block_out_channels: Tuple[int, ...] = (320, 640, 1280, 1280)
    layers_per_block: int = 2
    attn_levels: Tuple[bool, ...] = (True, True, True, False)
    cross_attention_dim: int = 768
    num_heads: int = 8
    norm_num_groups: int = 32
    norm_eps: float = 1e-5
    context_len: int = 77
    # LCM-distilled UNets (diffusers ``time_cond_proj_dim``, read by the reference loop at src/models.py:195-202): the time
    # embedding adds ``cond_proj(guidance embedding)`` to the timestep sinusoid.  None = no cond_proj (SD-1.5).  Declared as
    # an InitVar and kept as an instance attribute: ``dataclasses.asdict`` of a config then still builds the oracle's
    # ``UNetConfig`` (which has no such field), and ``dataclasses.replace`` carries the value over.
    time_cond_proj_dim: InitVar[Optional[int]] = None
    # IP-Adapter image prompts (diffusers ``ImageProjection`` + ``IPAdapterAttnProcessor2_0``, the plain ip-adapter_sd15
    # family): width E of ``image_embeds`` (1024 for the published adapter), None = no adapter.  The UNet then carries the
    # token projection and ``to_k_ip`` / ``to_v_ip`` of every attn2 layer (``param_shapes``).  ``ip_adapter_tokens`` is the
    # number of image tokens per sample: IP_ADAPTER_TOKENS with an adapter, else None.  InitVars like the field above.
    ip_adapter_embed_dim: InitVar[Optional[int]] = None
    ip_adapter_tokens: InitVar[Optional[int]] = None
    # Stable Diffusion 2.x.  ``num_heads_per_level``: the head COUNT of the transformer blocks per resolution level
    # ((5, 10, 20, 20): head dim 64 everywhere; diffusers' ``attention_head_dim`` list), None = ``num_heads`` at every level.
    # The mid block uses the last level's count, the up blocks mirror the down blocks (``heads_per_level``).
    # ``use_linear_projection``: ``proj_in`` / ``proj_out`` are Linear layers, weights [C, C] instead of [C, C, 1, 1]; in the
    # token-major layout both are the same GEMM, so only the shape a state dict is checked against differs.  InitVars like the
    # fields above.
    num_heads_per_level: InitVar[Optional[Tuple[int, ...]]] = None
    use_linear_projection: InitVar[bool] = False

    def __post_init__(self, time_cond_proj_dim, ip_adapter_embed_dim, ip_adapter_tokens, num_heads_per_level=None,
                      use_linear_projection=False):
        hp = num_heads_per_level
        if hp is not None:
            hp = tuple(hp)
            if len(hp) != len(self.block_out_channels) or any(isinstance(v, bool) or int(v) != v or int(v) <= 0 for v in hp):
                raise ValueError(f"num_heads_per_level={num_heads_per_level!r}: one positive integer per level "
                                 f"({len(self.block_out_channels)}) or None")
            hp = tuple(int(v) for v in hp)
        self.num_heads_per_level = hp
        if not isinstance(use_linear_projection, bool):
            raise ValueError(f"use_linear_projection={use_linear_projection!r}: a bool")
        self.use_linear_projection = use_linear_projection
        if time_cond_proj_dim is not None and (isinstance(time_cond_proj_dim, bool) or int(time_cond_proj_dim) <= 0
                                               or int(time_cond_proj_dim) != time_cond_proj_dim):
            raise ValueError(f"time_cond_proj_dim={time_cond_proj_dim!r}: a positive integer or None")
        self.time_cond_proj_dim = None if time_cond_proj_dim is None else int(time_cond_proj_dim)
        e, t = ip_adapter_embed_dim, ip_adapter_tokens
        if e is None:
            if t is not None:
                raise ValueError(f"ip_adapter_tokens={t!r} without ip_adapter_embed_dim")
            self.ip_adapter_embed_dim = self.ip_adapter_tokens = None
            return
        if isinstance(e, bool) or int(e) != e or int(e) <= 0 or int(e) % 64:
            raise ValueError(f"ip_adapter_embed_dim={e!r}: a positive multiple of 64 or None")
        if t is not None and (isinstance(t, bool) or t != IP_ADAPTER_TOKENS):
            raise NotImplementedError(f"ip_adapter_tokens={t!r}: {IP_ADAPTER_TOKENS} image tokens are built (the plain "
                                      "ip-adapter_sd15 family; the 'plus' / 'full-face' adapters have 16 or 257)")
        self.ip_adapter_embed_dim, self.ip_adapter_tokens = int(e), IP_ADAPTER_TOKENS

    def __eq__(self, other):            # (the generated one compares fields only)
        if other.__class__ is not self.__class__:
            return NotImplemented
        a, b = _shared_fields(self), _shared_fields(other)
        a.pop("num_heads"), b.pop("num_heads")          # (compared through heads_per_level)
        return (a == b and self.heads_per_level == other.heads_per_level
                and self.use_linear_projection == other.use_linear_projection
                and self.time_cond_proj_dim == other.time_cond_proj_dim
                and self.ip_adapter_embed_dim == other.ip_adapter_embed_dim)

    @property
    def heads_per_level(self) -> Tuple[int, ...]:
        """The head count of every level: ``num_heads_per_level``, or ``num_heads`` at each."""
        return self.num_heads_per_level or (self.num_heads,) * len(self.block_out_channels)


IP_ADAPTER_TOKENS = 4

# Stable Diffusion 2.x (stable-diffusion-2-base / -2 / -2-1-base / -2-1 / -2-inpainting): head dim 64 at every level, the
# OpenCLIP ViT-H text tower's 1024-wide context, Linear proj_in / proj_out
SD2_HEADS = (5, 10, 20, 20)
SD2_CONTEXT_DIM = 1024


def sd2_unet_config(sample_size: int = 96, in_channels: int = 4) -> "UNetConfig":
    """The UNet of the Stable Diffusion 2.x family (``sample_size`` 96 for the 768-pixel checkpoints, 64 for the ``-base``
    ones; ``in_channels`` 9 for ``-2-inpainting``)."""
    return UNetConfig(sample_size=int(sample_size), in_channels=int(in_channels), cross_attention_dim=SD2_CONTEXT_DIM,
                      num_heads=SD2_HEADS[0], num_heads_per_level=SD2_HEADS, use_linear_projection=True)


def check_projection_layout(cfg: "UNetConfig", sd) -> None:
    """A checkpoint's ``use_linear_projection`` and the rank of its ``proj_in`` / ``proj_out`` weights must agree ([C, C] for
    Linear, [C, C, 1, 1] for the 1x1 conv): one whose config and weights disagree is refused by name, not reshaped."""
    want = 2 if cfg.use_linear_projection else 4
    for name, v in sd.items():
        if name.endswith(("proj_in.weight", "proj_out.weight")) and v.dim() != want:
            raise NotImplementedError(f"unet config use_linear_projection={cfg.use_linear_projection!r}, but {name} has shape "
                                      f"{tuple(v.shape)}: the checkpoint's config and weights disagree")
IP_PROJ = "encoder_hid_proj.image_projection_layers.0."       # diffusers: unet.encoder_hid_proj of one loaded adapter


def param_shapes(cfg: UNetConfig) -> List[Tuple[str, Tuple[int, ...]]]:
    """(name, shape) of every UNet parameter in forward order."""
    out: List[Tuple[str, Tuple[int, ...]]] = []
    add = lambda n, s: out.append((n, tuple(s)))
    c0 = cfg.block_out_channels[0]
    temb = 4 * c0
    nl = len(cfg.block_out_channels)

    def resnet(p, cin, cout):
        add(p + "norm1.weight", (cin,)); add(p + "norm1.bias", (cin,))
        add(p + "conv1.weight", (cout, cin, 3, 3)); add(p + "conv1.bias", (cout,))
        add(p + "time_emb_proj.weight", (cout, temb)); add(p + "time_emb_proj.bias", (cout,))
        add(p + "norm2.weight", (cout,)); add(p + "norm2.bias", (cout,))
        add(p + "conv2.weight", (cout, cout, 3, 3)); add(p + "conv2.bias", (cout,))
        if cin != cout:
            add(p + "conv_shortcut.weight", (cout, cin, 1, 1)); add(p + "conv_shortcut.bias", (cout,))

    def transformer(p, c):
        ctx = cfg.cross_attention_dim
        add(p + "norm.weight", (c,)); add(p + "norm.bias", (c,))
        proj = (c, c) if cfg.use_linear_projection else (c, c, 1, 1)
        add(p + "proj_in.weight", proj); add(p + "proj_in.bias", (c,))
        t = p + "transformer_blocks.0."
        for i in (1, 2, 3):
            add(t + f"norm{i}.weight", (c,)); add(t + f"norm{i}.bias", (c,))
        add(t + "attn1.to_q.weight", (c, c)); add(t + "attn1.to_k.weight", (c, c)); add(t + "attn1.to_v.weight", (c, c))
        add(t + "attn1.to_out.0.weight", (c, c)); add(t + "attn1.to_out.0.bias", (c,))
        add(t + "attn2.to_q.weight", (c, c)); add(t + "attn2.to_k.weight", (c, ctx)); add(t + "attn2.to_v.weight", (c, ctx))
        add(t + "attn2.to_out.0.weight", (c, c)); add(t + "attn2.to_out.0.bias", (c,))
        if cfg.ip_adapter_embed_dim is not None:
            add(t + "attn2.processor.to_k_ip.0.weight", (c, ctx)); add(t + "attn2.processor.to_v_ip.0.weight", (c, ctx))
        add(t + "ff.net.0.proj.weight", (8 * c, c)); add(t + "ff.net.0.proj.bias", (8 * c,))
        add(t + "ff.net.2.weight", (c, 4 * c)); add(t + "ff.net.2.bias", (c,))
        add(p + "proj_out.weight", proj); add(p + "proj_out.bias", (c,))

    add("time_embedding.linear_1.weight", (temb, c0)); add("time_embedding.linear_1.bias", (temb,))
    if cfg.time_cond_proj_dim is not None:
        add("time_embedding.cond_proj.weight", (c0, cfg.time_cond_proj_dim))
    add("time_embedding.linear_2.weight", (temb, temb)); add("time_embedding.linear_2.bias", (temb,))
    add("conv_in.weight", (c0, cfg.in_channels, 3, 3)); add("conv_in.bias", (c0,))
    ch = c0
    skip_ch = [c0]
    for i in range(nl):
        co = cfg.block_out_channels[i]
        for j in range(cfg.layers_per_block):
            resnet(f"down_blocks.{i}.resnets.{j}.", ch, co)
            ch = co
            if cfg.attn_levels[i]:
                transformer(f"down_blocks.{i}.attentions.{j}.", co)
            skip_ch.append(co)
        if i < nl - 1:
            add(f"down_blocks.{i}.downsamplers.0.conv.weight", (co, co, 3, 3))
            add(f"down_blocks.{i}.downsamplers.0.conv.bias", (co,))
            skip_ch.append(co)
    resnet("mid_block.resnets.0.", ch, ch)
    transformer("mid_block.attentions.0.", ch)
    resnet("mid_block.resnets.1.", ch, ch)
    for i in range(nl):
        lev = nl - 1 - i
        co = cfg.block_out_channels[lev]
        for j in range(cfg.layers_per_block + 1):
            resnet(f"up_blocks.{i}.resnets.{j}.", ch + skip_ch.pop(), co)
            ch = co
            if cfg.attn_levels[lev]:
                transformer(f"up_blocks.{i}.attentions.{j}.", co)
        if i < nl - 1:
            add(f"up_blocks.{i}.upsamplers.0.conv.weight", (co, co, 3, 3))
            add(f"up_blocks.{i}.upsamplers.0.conv.bias", (co,))
    add("conv_norm_out.weight", (c0,)); add("conv_norm_out.bias", (c0,))
    add("conv_out.weight", (cfg.out_channels, c0, 3, 3)); add("conv_out.bias", (cfg.out_channels,))
    if cfg.ip_adapter_embed_dim is not None:
        td = cfg.ip_adapter_tokens * cfg.cross_attention_dim
        add(IP_PROJ + "image_embeds.weight", (td, cfg.ip_adapter_embed_dim)); add(IP_PROJ + "image_embeds.bias", (td,))
        add(IP_PROJ + "norm.weight", (cfg.cross_attention_dim,)); add(IP_PROJ + "norm.bias", (cfg.cross_attention_dim,))
    return out


def attn2_prefixes(cfg: UNetConfig) -> List[str]:
    """The ``...transformer_blocks.0.attn2.`` prefixes in the order of diffusers' ``unet.attn_processors``: all of
    ``down_blocks``, then all of ``up_blocks``, then ``mid_block`` (module registration order, NOT forward order).  An
    IP-Adapter checkpoint numbers the processors in that order, attn1 and attn2 alternating: the i-th prefix here is
    its key ``2 i + 1`` (1, 3, ..., 31 for SD-1.5)."""
    nl = len(cfg.block_out_channels)
    out = []
    for i in range(nl):
        if cfg.attn_levels[i]:
            out += [f"down_blocks.{i}.attentions.{j}.transformer_blocks.0.attn2." for j in range(cfg.layers_per_block)]
    for i in range(nl):
        if cfg.attn_levels[nl - 1 - i]:
            out += [f"up_blocks.{i}.attentions.{j}.transformer_blocks.0.attn2." for j in range(cfg.layers_per_block + 1)]
    out.append("mid_block.attentions.0.transformer_blocks.0.attn2.")
    return out


def ip_adapter_param_shapes(cfg: UNetConfig) -> List[Tuple[str, Tuple[int, ...]]]:
    """(name, shape) of the parameters an IP-Adapter adds to the UNet (``cfg.ip_adapter_embed_dim`` set)."""
    plain = {n for n, _ in param_shapes(without_ip_adapter(cfg))}
    return [(n, s) for n, s in param_shapes(cfg) if n not in plain]


def without_ip_adapter(cfg: UNetConfig) -> UNetConfig:
    import dataclasses
    return dataclasses.replace(cfg, ip_adapter_embed_dim=None, ip_adapter_tokens=None)


IP_ADAPTER_SEED_OFFSET = 104729


def make_synthetic_ip_adapter_state_dict(cfg: UNetConfig, seed: int = 1234, gain: float = 1.0) -> Dict[str, torch.Tensor]:
    """Seeded IP-Adapter-shaped weights under the UNet's names (``ip_adapter_param_shapes``), fp32 on the bf16 grid, from a
    generator of their own: linear weights ~ N(0, gain^2 / fan_in), the projection bias ~ N(0, 0.05^2), the token LayerNorm
    1 + N(0, 0.1^2) / N(0, 0.1^2).  Stands in for a hub adapter (no weights exist offline) and serves the tests."""
    if cfg.ip_adapter_embed_dim is None:
        raise ValueError("make_synthetic_ip_adapter_state_dict: the config has no ip_adapter_embed_dim")
    g = torch.Generator().manual_seed(IP_ADAPTER_SEED_OFFSET + int(seed))
    sd = {}
    for name, shape in ip_adapter_param_shapes(cfg):
        if name.endswith("norm.weight"):
            t = 1.0 + 0.1 * torch.randn(shape, generator=g)
        elif name.endswith("norm.bias"):
            t = 0.1 * torch.randn(shape, generator=g)
        elif name.endswith(".bias"):
            t = 0.05 * torch.randn(shape, generator=g)
        else:
            t = torch.randn(shape, generator=g) * (gain / math.sqrt(shape[1]))
        sd[name] = t.to(torch.bfloat16).float()
    return sd


def to_upstream_ip_adapter(sd: Dict[str, torch.Tensor], cfg: UNetConfig) -> Dict[str, Dict[str, torch.Tensor]]:
    """The inverse of ``map_ip_adapter_state_dict``: UNet names -> the checkpoint's two groups (what ``ip-adapter_sd15.bin``
    holds).  Tests and tools write synthetic checkpoints with it."""
    out = {"image_proj": {"proj.weight": sd[IP_PROJ + "image_embeds.weight"], "proj.bias": sd[IP_PROJ + "image_embeds.bias"],
                          "norm.weight": sd[IP_PROJ + "norm.weight"], "norm.bias": sd[IP_PROJ + "norm.bias"]},
           "ip_adapter": {}}
    for i, p in enumerate(attn2_prefixes(cfg)):
        out["ip_adapter"][f"{2 * i + 1}.to_k_ip.weight"] = sd[p + "processor.to_k_ip.0.weight"]
        out["ip_adapter"][f"{2 * i + 1}.to_v_ip.weight"] = sd[p + "processor.to_v_ip.0.weight"]
    return out


def map_ip_adapter_state_dict(groups: Dict[str, Dict[str, torch.Tensor]], cfg: UNetConfig):
    """An IP-Adapter checkpoint's groups ``image_proj`` / ``ip_adapter`` (upstream layout) -> (UNet-named fp32 state dict,
    embed dim E).  ``ip_adapter`` keys are ``"{k}.to_k_ip.weight"`` / ``"{k}.to_v_ip.weight"`` with k = 1, 3, ...: k counts
    ``unet.attn_processors`` -- attn1 / attn2 alternating over all of down_blocks, then all of up_blocks, then mid_block
    (``attn2_prefixes``), which is NOT the forward order.  Missing keys raise ``KeyError``, wrong shapes ``ValueError``, and
    the projections this build does not run (Resampler / MLP: the 'plus' and 'full-face' adapters) ``NotImplementedError``,
    each naming the key."""
    for grp in ("image_proj", "ip_adapter"):
        if grp not in groups:
            raise KeyError(f"IP-Adapter checkpoint lacks the group {grp!r}")
    proj, ipa = groups["image_proj"], groups["ip_adapter"]
    if any(k.startswith(("latents", "proj_in", "layers.", "proj.0", "proj.3", "perceiver_resampler")) for k in proj):
        raise NotImplementedError("IP-Adapter image_proj is a Resampler / MLP projection (the 'plus' / 'full-face' adapters, 16 or "
                                  "257 image tokens): only the plain ImageProjection (proj + norm, 4 tokens) is built")
    for k in ("proj.weight", "proj.bias", "norm.weight", "norm.bias"):
        if k not in proj:
            raise KeyError(f"IP-Adapter checkpoint lacks image_proj.{k}")
    cd = cfg.cross_attention_dim
    w = proj["proj.weight"]
    if w.dim() != 2 or w.shape[0] % cd:
        raise ValueError(f"image_proj.proj.weight: expected [T * {cd}, E], got {tuple(w.shape)}")
    tokens, e = w.shape[0] // cd, int(w.shape[1])
    if tokens != IP_ADAPTER_TOKENS:
        raise NotImplementedError(f"image_proj.proj.weight {tuple(w.shape)}: {tokens} image tokens; {IP_ADAPTER_TOKENS} are built")
    want = {"proj.bias": (tokens * cd,), "norm.weight": (cd,), "norm.bias": (cd,)}
    for k, shp in want.items():
        if tuple(proj[k].shape) != shp:
            raise ValueError(f"image_proj.{k}: expected shape {shp}, got {tuple(proj[k].shape)}")
    f32 = lambda t: t.detach().to("cpu", torch.float32).contiguous()
    sd = {IP_PROJ + "image_embeds.weight": f32(w), IP_PROJ + "image_embeds.bias": f32(proj["proj.bias"]),
          IP_PROJ + "norm.weight": f32(proj["norm.weight"]), IP_PROJ + "norm.bias": f32(proj["norm.bias"])}
    chan = {n[: -len("to_q.weight")]: s[0] for n, s in param_shapes(without_ip_adapter(cfg)) if n.endswith("attn2.to_q.weight")}
    for i, p in enumerate(attn2_prefixes(cfg)):
        for which in ("to_k_ip", "to_v_ip"):
            k = f"{2 * i + 1}.{which}.weight"
            if k not in ipa:
                raise KeyError(f"IP-Adapter checkpoint lacks ip_adapter.{k} (the attn2 of {p[:-1]})")
            if tuple(ipa[k].shape) != (chan[p], cd):
                raise ValueError(f"ip_adapter.{k}: expected shape {(chan[p], cd)} (the attn2 of {p[:-1]}), got {tuple(ipa[k].shape)}")
            sd[p + f"processor.{which}.0.weight"] = f32(ipa[k])
    return sd, e


def load_ip_adapter_state_dict(path: str, cfg: UNetConfig):
    """A LOCAL IP-Adapter file in the upstream layout -> ``map_ip_adapter_state_dict``'s result: a ``.safetensors`` with the
    ``image_proj.`` / ``ip_adapter.`` key prefixes, or a ``.bin`` (``torch.save`` of the nested dict).  Never fetches."""
    if not os.path.isfile(path):
        raise FileNotFoundError(f"no IP-Adapter file at {path!r}")
    if path.endswith(".safetensors"):
        from safetensors.torch import load_file
        groups: Dict[str, Dict[str, torch.Tensor]] = {"image_proj": {}, "ip_adapter": {}}
        for k, v in load_file(path).items():
            grp, _, rest = k.partition(".")
            if grp in groups:
                groups[grp][rest] = v
        groups = {g: d for g, d in groups.items() if d}
    else:
        groups = torch.load(path, map_location="cpu", weights_only=True)
        if not isinstance(groups, dict):
            raise ValueError(f"{path!r}: an IP-Adapter .bin holds a dict with the groups 'image_proj' and 'ip_adapter'")
    return map_ip_adapter_state_dict(groups, cfg)


# ---- ControlNet (diffusers ControlNetModel) ----------------------------------------------------------------
CONTROLNET_EMBED_CHANNELS = (16, 32, 96, 256)        # conditioning_embedding_out_channels of the published SD-1.5 ControlNets
CONTROLNET_SHARED_FIELDS = ("block_out_channels", "layers_per_block", "attn_levels", "cross_attention_dim", "heads_per_level",
                            "norm_num_groups", "norm_eps", "context_len")       # heads_per_level: num_heads where no level differs
CONTROLNET_SEED_OFFSET = 15485863
CONTROLNET_SYNTHETIC_GAIN = 0.5                      # make_synthetic_controlnet_state_dict: see tests/test_controlnet_cpu.py


@dataclass
class ControlNetConfig:
    """``unet``: the fields a ControlNet shares with the UNet it is paired with (4 input channels, no IP-Adapter; its
    ``sample_size`` is only the default latent size); ``conditioning_embedding_out_channels``: the widths of the
    conditioning embedding's conv chain."""
    unet: UNetConfig
    conditioning_embedding_out_channels: Tuple[int, ...] = CONTROLNET_EMBED_CHANNELS

    def __post_init__(self):
        e = tuple(int(v) for v in self.conditioning_embedding_out_channels)
        if len(e) != 4 or any(v <= 0 or v % 8 for v in e):
            raise NotImplementedError(f"conditioning_embedding_out_channels={e}: four positive multiples of 8 are built "
                                      f"(the published ControlNets have {CONTROLNET_EMBED_CHANNELS})")
        self.conditioning_embedding_out_channels = e
        if self.unet.in_channels != 4 or self.unet.ip_adapter_embed_dim is not None:
            raise NotImplementedError("a ControlNet has 4 input channels and no IP-Adapter")


def controlnet_config_for(unet_cfg: UNetConfig, embed_channels=CONTROLNET_EMBED_CHANNELS) -> ControlNetConfig:
    """The ControlNet config that pairs with ``unet_cfg`` (an inpainting UNet's ControlNet still reads 4 channels; the
    ControlNet has no ``cond_proj``: upstream's pipeline passes it no ``timestep_cond``)."""
    import dataclasses
    base = dataclasses.replace(without_ip_adapter(unet_cfg), in_channels=4, out_channels=4, time_cond_proj_dim=None)
    return ControlNetConfig(unet=base, conditioning_embedding_out_channels=tuple(embed_channels))


def check_controlnet_pairs(cn: ControlNetConfig, unet_cfg: UNetConfig) -> None:
    """The fields a ControlNet shares with its UNet must agree: the residuals are added to the UNet's skip tensors."""
    for f in CONTROLNET_SHARED_FIELDS:
        a, b = getattr(cn.unet, f), getattr(unet_cfg, f)
        if (tuple(a) if isinstance(a, (list, tuple)) else a) != (tuple(b) if isinstance(b, (list, tuple)) else b):
            raise ValueError(f"controlnet config {f}={a!r} does not match the UNet it is paired with ({f}={b!r})")


def read_controlnet_config(c: dict, unet_config: Optional[UNetConfig] = None) -> ControlNetConfig:
    """The dict of a diffusers ControlNet ``config.json`` -> ``ControlNetConfig``.  Read: ``conditioning_embedding_out_channels``,
    ``controlnet_conditioning_channel_order`` ("rgb" only), ``global_pool_conditions`` (false only), ``conditioning_channels``
    (3 only) and the fields shared with the UNet through ``read_unet_config`` (a ControlNet has no up blocks: they are taken
    as the mirror of its down blocks).  With ``unet_config`` the shared fields must agree with it; anything else is refused
    by name."""
    order = c.get("controlnet_conditioning_channel_order", "rgb")
    if order != "rgb":
        raise NotImplementedError(f"controlnet config controlnet_conditioning_channel_order={order!r}: 'rgb' is built")
    if c.get("global_pool_conditions", False) is not False:
        raise NotImplementedError(f"controlnet config global_pool_conditions={c['global_pool_conditions']!r}: false is built")
    if c.get("conditioning_channels", 3) != 3:
        raise NotImplementedError(f"controlnet config conditioning_channels={c['conditioning_channels']!r}: 3 (an rgb image) is built")
    if c.get("in_channels", 4) != 4:
        raise NotImplementedError(f"controlnet config in_channels={c['in_channels']!r}: 4 is built")
    down = list(c.get("down_block_types", ["CrossAttnDownBlock2D"] * 3 + ["DownBlock2D"]))
    mirror = ["CrossAttnUpBlock2D" if d == "CrossAttnDownBlock2D" else "UpBlock2D" for d in reversed(down)]
    shared = {k: v for k, v in c.items() if k not in ("time_cond_proj_dim", "up_block_types")}
    shared["up_block_types"] = mirror
    ucfg = read_unet_config(shared)
    cn = ControlNetConfig(unet=ucfg, conditioning_embedding_out_channels=tuple(
        c.get("conditioning_embedding_out_channels", CONTROLNET_EMBED_CHANNELS)))
    if unet_config is not None:
        check_controlnet_pairs(cn, unet_config)
    return cn


def controlnet_cond_embedding_convs(cn: ControlNetConfig) -> List[Tuple[str, int, int, int]]:
    """(prefix, cin, cout, stride) of ControlNetConditioningEmbedding's eight 3x3 convs; SiLU follows all but the last."""
    e, p = cn.conditioning_embedding_out_channels, "controlnet_cond_embedding."
    out = [(p + "conv_in.", 3, e[0], 1)]
    for i in range(3):
        out += [(p + f"blocks.{2 * i}.", e[i], e[i], 1), (p + f"blocks.{2 * i + 1}.", e[i], e[i + 1], 2)]
    return out + [(p + "conv_out.", e[3], cn.unet.block_out_channels[0], 1)]


def controlnet_residual_shapes(cn, height: int, width: int) -> List[Tuple[int, int, int]]:
    """(channels, h, w) of the thirteen residuals at a latent ``height`` x ``width`` (``cn``: a ControlNetConfig or the UNet's
    config), in diffusers' order: conv_in, per level its blocks then its downsampler, the mid block last."""
    u = cn.unet if isinstance(cn, ControlNetConfig) else cn
    nl, h, w = len(u.block_out_channels), int(height), int(width)
    out = [(u.block_out_channels[0], h, w)]
    for i in range(nl):
        out += [(u.block_out_channels[i], h, w)] * u.layers_per_block
        if i < nl - 1:
            h, w = h // 2, w // 2
            out.append((u.block_out_channels[i], h, w))
    return out + [(u.block_out_channels[-1], h, w)]


def controlnet_param_shapes(cn: ControlNetConfig) -> List[Tuple[str, Tuple[int, ...]]]:
    """(name, shape) of every ControlNet parameter: the UNet's time embedding, conv_in, down blocks and mid block under the
    UNet's names, then the conditioning embedding and the zero convs."""
    out = [(n, s) for n, s in param_shapes(cn.unet)
           if not n.startswith(("up_blocks.", "conv_norm_out.", "conv_out."))]
    for p, cin, cout, _ in controlnet_cond_embedding_convs(cn):
        out += [(p + "weight", (cout, cin, 3, 3)), (p + "bias", (cout,))]
    res = controlnet_residual_shapes(cn, 8, 8)
    for i, (c, _, _) in enumerate(res[:-1]):
        out += [(f"controlnet_down_blocks.{i}.weight", (c, c, 1, 1)), (f"controlnet_down_blocks.{i}.bias", (c,))]
    c = res[-1][0]
    return out + [("controlnet_mid_block.weight", (c, c, 1, 1)), ("controlnet_mid_block.bias", (c,))]


def make_synthetic_controlnet_state_dict(cn: ControlNetConfig, seed: int = 1234,
                                         gain: float = CONTROLNET_SYNTHETIC_GAIN) -> Dict[str, torch.Tensor]:
    """Seeded ControlNet-shaped weights on the bf16 grid from a generator of their own.  The encoder half is drawn like the
    UNet's (``make_synthetic_state_dict``'s rules).  Upstream initialises the zero convs and the embedding's ``conv_out`` to
    ZERO: a fresh ControlNet is a no-op.  Here the zero convs are N(0, gain^2 / fan_in) with biases N(0, 0.05^2), so that the
    residuals move the UNet's output (tests/test_controlnet_cpu.py fixes ``gain``), and the embedding's convs are
    N(0, 2 / fan_in), its ``conv_out`` N(0, 9 / fan_in) (the strided SiLU chain shrinks a [0, 1] image): the embedding then is a third
    of conv_in's output in size, so a wrong control image shows in every residual."""
    g = torch.Generator().manual_seed(CONTROLNET_SEED_OFFSET + int(seed))
    sd: Dict[str, torch.Tensor] = {}
    for name, shape in controlnet_param_shapes(cn):
        leaf = name.rsplit(".", 2)[-2]
        is_norm = leaf.startswith("norm")
        zero_conv = name.startswith(("controlnet_down_blocks.", "controlnet_mid_block."))
        if name.endswith(".bias"):
            t = torch.randn(shape, generator=g) * (0.1 if is_norm else 0.05)
        elif is_norm:
            t = 1.0 + 0.1 * torch.randn(shape, generator=g)
        else:
            fan_in = math.prod(shape[1:])
            k = gain if zero_conv else 3.0 if name.startswith("controlnet_cond_embedding.conv_out.") else \
                math.sqrt(2.0) if name.startswith("controlnet_cond_embedding.") else 1.0
            t = torch.randn(shape, generator=g) * (k / math.sqrt(fan_in))
        sd[name] = t.to(torch.bfloat16).float()
    return sd


def load_controlnet(path: str, unet_config: Optional[UNetConfig] = None):
    """A LOCAL ControlNet directory in the upstream layout (``config.json`` and ``diffusion_pytorch_model.safetensors`` or
    ``.bin``) -> (ControlNetConfig, fp32 state dict).  Never fetches."""
    import json
    cfile = os.path.join(path, "config.json")
    if not os.path.isfile(cfile):
        raise FileNotFoundError(f"no ControlNet config at {cfile!r}")
    with open(cfile, encoding="utf-8") as f:
        cn = read_controlnet_config(json.load(f), unet_config)
    st, bn = os.path.join(path, "diffusion_pytorch_model.safetensors"), os.path.join(path, "diffusion_pytorch_model.bin")
    if os.path.isfile(st):
        from safetensors.torch import load_file
        sd = load_file(st)
    elif os.path.isfile(bn):
        sd = torch.load(bn, map_location="cpu", weights_only=True)
    else:
        raise FileNotFoundError(f"no ControlNet weights under {path!r} (diffusion_pytorch_model.safetensors / .bin)")
    return cn, {k: v.float() for k, v in sd.items()}


def control_keep(num_steps: int, control_guidance_start: float = 0.0, control_guidance_end: float = 1.0) -> List[float]:
    """``controlnet_keep`` of StableDiffusionControlNetPipeline: step i of N keeps the ControlNet unless
    ``i / N < start or (i + 1) / N > end``."""
    n = int(num_steps)
    return [1.0 - float(i / n < control_guidance_start or (i + 1) / n > control_guidance_end) for i in range(n)]


_SYNTHETIC_CACHE: Dict[tuple, Dict[str, torch.Tensor]] = {}


def make_synthetic_state_dict(cfg: UNetConfig, seed: int = 1234) -> Dict[str, torch.Tensor]:
    """Seeded SD-1.5-shaped weights, fp32 values already on the bf16 grid.

    Conv/linear weights ~ N(0, 1/fan_in) (unit gain, so activations stay O(1) through the
    normalised blocks), biases ~ N(0, 0.05^2), norm gains 1 + N(0, 0.1^2), norm shifts
    N(0, 0.1^2) (non-trivial affine so parity tests exercise it).  Rounding to bf16 here means
    the CPU oracle and the HIP path consume bit-identical parameters.

    The values do not depend on ``sample_size`` or on the head counts (no parameter shape does), and a
    ``use_linear_projection`` config draws the same numbers into [C, C] ``proj_in`` / ``proj_out``; generating 0.86 G Gaussians takes ~10 s, so the
    result is cached per (architecture, seed) for the life of the process and every call returns a NEW dict over the same
    read-only tensors (callers replace entries -- LoRA fusion, tests -- and never write into a tensor).

    ``time_cond_proj_dim`` set: ``time_embedding.cond_proj.weight`` is drawn from a generator of its own (seed
    ``COND_PROJ_SEED_OFFSET + seed``), so every other parameter is bit-identical to the plain config's.
    """
    key = (cfg.in_channels, cfg.out_channels, tuple(cfg.block_out_channels), cfg.layers_per_block, tuple(cfg.attn_levels),
           cfg.cross_attention_dim, bool(cfg.use_linear_projection), int(seed))
    if key in _SYNTHETIC_CACHE:
        return _with_cond_proj(dict(_SYNTHETIC_CACHE[key]), cfg, seed)
    g = torch.Generator().manual_seed(seed)
    sd: Dict[str, torch.Tensor] = {}
    plain = UNetConfig(**_shared_fields(cfg), use_linear_projection=cfg.use_linear_projection)     # (without cond_proj)
    for name, shape in param_shapes(plain):
        leaf = name.rsplit(".", 2)[-2]
        is_norm = leaf.startswith("norm") or leaf == "conv_norm_out"
        if name.endswith(".bias"):
            t = torch.randn(shape, generator=g) * (0.1 if is_norm else 0.05)
        elif is_norm:
            t = 1.0 + 0.1 * torch.randn(shape, generator=g)
        else:
            fan_in = math.prod(shape[1:])
            t = torch.randn(shape, generator=g) / math.sqrt(fan_in)
        sd[name] = t.to(torch.bfloat16).float()
    if len(_SYNTHETIC_CACHE) >= 2:            # (3.4 GB per SD-1.5-sized entry)
        _SYNTHETIC_CACHE.pop(next(iter(_SYNTHETIC_CACHE)))
    _SYNTHETIC_CACHE[key] = sd
    return _with_cond_proj(dict(sd), cfg, seed)


COND_PROJ_SEED_OFFSET = 7919


def _shared_fields(cfg: UNetConfig) -> dict:
    """The config's dataclass fields (everything but ``time_cond_proj_dim``)."""
    import dataclasses
    return {f.name: getattr(cfg, f.name) for f in dataclasses.fields(cfg)}


def _with_cond_proj(sd: Dict[str, torch.Tensor], cfg: UNetConfig, seed: int) -> Dict[str, torch.Tensor]:
    d = cfg.time_cond_proj_dim
    if d is not None:
        g = torch.Generator().manual_seed(COND_PROJ_SEED_OFFSET + int(seed))
        shape = (cfg.block_out_channels[0], d)
        sd["time_embedding.cond_proj.weight"] = (torch.randn(shape, generator=g) / math.sqrt(d)).to(torch.bfloat16).float()
    return sd


def load_scheduler_config(model_dir: str) -> dict:
    """The checkpoint's scheduler config: ``scheduler/scheduler_config.json`` of a local diffusers directory over the
    SD-1.5 defaults (``schedulers.SD15_SCHEDULER_CONFIG``).  Keys starting with ``_`` are dropped except ``_class_name``
    (the checkpoint's scheduler class, ``schedulers.checkpoint_scheduler_name``).  No file: the SD-1.5 config."""
    import json
    from .schedulers import SD15_SCHEDULER_CONFIG
    cfg = dict(SD15_SCHEDULER_CONFIG)
    path = os.path.join(model_dir, "scheduler", "scheduler_config.json")
    if os.path.isfile(path):
        with open(path) as f:
            raw = json.load(f)
        cfg.update({k: v for k, v in raw.items() if not k.startswith("_") or k == "_class_name"})
    return cfg


def load_unet_config(model_dir: str) -> "UNetConfig | None":
    """``<dir>/unet/config.json`` of a LOCAL diffusers checkpoint -> ``UNetConfig`` (None if the file is absent: the
    SD-1.5 defaults then apply).  Only the keys this build implements are read; a checkpoint that needs anything else
    (another block type, class or added embeddings, several transformer blocks per layer, an activation other than silu)
    is refused here rather than mis-run.  Stable Diffusion 2.x configs (per-level head counts, ``use_linear_projection``,
    ``upcast_attention``) are read."""
    import json
    for cand in (os.path.join(model_dir, "unet", "config.json"), os.path.join(model_dir, "config.json")):
        if os.path.isfile(cand):
            with open(cand) as f:
                return read_unet_config(json.load(f))
    return None


def read_unet_config(c: dict) -> UNetConfig:
    """The dict of a diffusers ``unet/config.json`` -> ``UNetConfig`` (``load_unet_config`` on an open file).
    ``in_channels``: 4, or 9 for an inpainting checkpoint ([latents | mask | masked-image latents]); any other value is
    refused by name."""
    cin = c.get("in_channels", 4)
    if isinstance(cin, bool) or cin not in (4, 9):
        raise NotImplementedError(f"unet config in_channels={cin!r}: 4 (text-to-image) and 9 (inpainting: latents | mask | "
                                  "masked-image latents) are built")
    down = list(c.get("down_block_types", ["CrossAttnDownBlock2D"] * 3 + ["DownBlock2D"]))
    up = list(c.get("up_block_types", ["UpBlock2D"] + ["CrossAttnUpBlock2D"] * 3))
    known = {"CrossAttnDownBlock2D": True, "DownBlock2D": False}
    if any(d not in known for d in down):
        raise NotImplementedError(f"down_block_types {down}: CrossAttnDownBlock2D / DownBlock2D are built")
    attn = tuple(known[d] for d in down)
    if [u == "CrossAttnUpBlock2D" for u in up] != list(reversed(attn)):
        raise NotImplementedError(f"up_block_types {up} do not mirror down_block_types {down}")
    # diffusers' rule: ``num_attention_heads`` wins where it is present and not null; otherwise ``attention_head_dim`` holds
    # the NUMBER of heads (SD-1.5 quirk), an int or one entry per level (SD 2.x: [5, 10, 20, 20])
    heads = c.get("num_attention_heads", None)
    hkey = "num_attention_heads"
    if heads is None:
        heads, hkey = c.get("attention_head_dim", 8), "attention_head_dim"
    per_level = None
    if isinstance(heads, (list, tuple)):
        if len(heads) != len(down) or any(isinstance(v, bool) or not isinstance(v, int) or v <= 0 for v in heads):
            raise NotImplementedError(f"unet config {hkey}={heads!r}: one positive integer per level ({len(down)}) or an integer")
        per_level = tuple(heads) if len(set(heads)) != 1 else None
        heads = heads[0]
    elif isinstance(heads, bool) or not isinstance(heads, int) or heads <= 0:
        raise NotImplementedError(f"unet config {hkey}={heads!r}: a positive integer or one per level")
    tpb = c.get("transformer_layers_per_block", 1)
    if tpb != 1 and not (isinstance(tpb, (list, tuple)) and all(v == 1 for v in tpb)):
        raise NotImplementedError(f"unet config transformer_layers_per_block={tpb!r}: one transformer block per layer is built")
    if c.get("num_class_embeds", None) is not None:
        raise NotImplementedError(f"unet config num_class_embeds={c['num_class_embeds']!r}: class conditioning is not built")
    for key in ("use_linear_projection", "upcast_attention"):
        if not isinstance(c.get(key, False), bool):
            raise NotImplementedError(f"unet config {key}={c[key]!r}: true or false")
    tcond = c.get("time_cond_proj_dim", None)
    if tcond is not None and (isinstance(tcond, bool) or not isinstance(tcond, int) or tcond <= 0):
        raise NotImplementedError(f"unet config time_cond_proj_dim={tcond!r}: a positive integer (LCM-distilled) or null")
    # ``upcast_attention`` (SD 2.1) is accepted and changes nothing: upstream's flag computes the scores in fp32 because fp16
    # scores overflow; here the scores ALWAYS accumulate in fp32 from bf16 operands and the softmax is fp32
    for key, want in (("act_fn", "silu"), ("flip_sin_to_cos", True), ("freq_shift", 0),
                      ("class_embed_type", None), ("addition_embed_type", None),
                      ("dual_cross_attention", False), ("only_cross_attention", False)):
        if c.get(key, want) != want:
            raise NotImplementedError(f"unet config {key}={c[key]!r}: this build implements {want!r}")
    return UNetConfig(sample_size=int(c.get("sample_size", 64)), in_channels=int(c.get("in_channels", 4)),
                      out_channels=int(c.get("out_channels", 4)),
                      block_out_channels=tuple(int(v) for v in c.get("block_out_channels", (320, 640, 1280, 1280))),
                      layers_per_block=int(c.get("layers_per_block", 2)), attn_levels=attn,
                      cross_attention_dim=int(c.get("cross_attention_dim", 768)), num_heads=int(heads),
                      norm_num_groups=int(c.get("norm_num_groups", 32)), norm_eps=float(c.get("norm_eps", 1e-5)),
                      time_cond_proj_dim=tcond, num_heads_per_level=per_level,
                      use_linear_projection=bool(c.get("use_linear_projection", False)))


def load_unet_state_dict(model_dir: str) -> Dict[str, torch.Tensor]:
    """Load a LOCAL diffusers UNet (``<dir>/unet/diffusion_pytorch_model.safetensors``).
    Never fetches: names that are not local directories raise."""
    from safetensors.torch import load_file
    for cand in (os.path.join(model_dir, "unet", "diffusion_pytorch_model.safetensors"),
                 os.path.join(model_dir, "diffusion_pytorch_model.safetensors")):
        if os.path.isfile(cand):
            return {k: v.float() for k, v in load_file(cand).items()}
    raise FileNotFoundError(
        f"no local UNet weights under {model_dir!r}; model names are network fetches and are "
        "unavailable offline -- use synthetic weights or point at a local diffusers directory")


def fuse_lora_state_dict(sd: Dict[str, torch.Tensor], lora_sd: Dict[str, torch.Tensor], scale: float = 1.0) -> int:
    """``pipe.load_lora_weights(...); pipe.fuse_lora()`` on the host copy of the UNet weights
    (``src/experiments/consistency_model.py:20-21``): ``W += scale * (alpha / r) * up @ down`` for every adapted
    module, linear or conv (3x3 ``down`` [r,I,kh,kw] with 1x1 ``up`` [O,r,1,1]).  Accepts the two layouts LoRA
    files for SD-1.5 come in [upstream-recall]: kohya (``lora_unet_<module with _>.lora_down/.lora_up.weight`` +
    ``.alpha``, what ``latent-consistency/lcm-lora-sdv1-5`` ships) and peft/diffusers
    (``unet.<module>.lora_A/.lora_B.weight``, alpha = r).  Text-encoder entries are ignored.  Returns the number of
    fused modules; raises if an adapted UNet module does not exist."""
    flat = {k[: -len(".weight")].replace(".", "_"): k for k in sd if k.endswith(".weight")}
    pairs = {}
    for k, v in lora_sd.items():
        if k.startswith("lora_te") or k.startswith("text_encoder."):
            continue
        if k.startswith("lora_unet_"):
            mod, _, leaf = k[len("lora_unet_"):].partition(".")
            target = flat.get(mod)
            if target is None:
                raise KeyError(f"LoRA module {mod!r} has no counterpart in the UNet")
            slot = {"lora_down.weight": "down", "lora_up.weight": "up", "alpha": "alpha"}.get(leaf)
        elif k.startswith("unet."):
            body = k[len("unet."):]
            for tag, slot_ in ((".lora_A.weight", "down"), (".lora_B.weight", "up"), (".lora.down.weight", "down"),
                               (".lora.up.weight", "up")):
                if body.endswith(tag):
                    target, slot = body[: -len(tag)] + ".weight", slot_
                    break
            else:
                continue
            if target not in sd:
                raise KeyError(f"LoRA module {target!r} has no counterpart in the UNet")
        else:
            continue
        if slot is not None:
            pairs.setdefault(target, {})[slot] = v
    n = 0
    for target, p in pairs.items():
        if "down" not in p or "up" not in p:
            raise KeyError(f"incomplete LoRA pair for {target}")
        down, up = p["down"].float(), p["up"].float()
        r = down.shape[0]
        alpha = float(p["alpha"]) if "alpha" in p else float(r)
        w = sd[target]
        delta = (up.reshape(up.shape[0], r) @ down.reshape(r, -1)).reshape(w.shape)
        sd[target] = (w.float() + scale * (alpha / r) * delta).to(torch.bfloat16).float()
        n += 1
    return n
