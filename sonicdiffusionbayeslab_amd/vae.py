"""``AutoencoderKL`` decoder and encoder on libsdhip -- SURVEY.md §8f "next" row 1.

Replaces ``self.vae.decode(latents / self.vae.config.scaling_factor)`` of the reference pipeline
(``src/models.py:287-302``): 2.5 TFLOP per 512x512 image, outside the reference's timed loop but what
turns latents into the ``[B,3,512,512]`` tensor the harness consumes (``output_type="pt"``).  Same
kernels as the UNet (implicit-GEMM conv with fused upsample, GroupNorm+SiLU, GEMM) plus a row softmax
for the single 512-wide attention head of the mid block.  No CPU fallback.

``HipVaeEncoder`` is ``AutoencoderKL.encode`` of diffusers 0.32.1 (upstream-recall, like the decoder): what
``StableDiffusionImg2ImgPipeline.prepare_latents`` runs on the input picture.  Entry conv (fp32 image in, ``2x - 1`` in the
load), the stride-2 downsamplers padded right / bottom only, and the exit (conv_out + quant_conv + the posterior sample) are
kernels of their own; the resnets and the mid attention run on the decoder's ops.
"""
from __future__ import annotations

import ctypes as C
import dataclasses
import math
import os
from dataclasses import dataclass
from typing import Dict, List, Optional, Tuple

import torch

from . import _lib
from .handle import HipHandle, Workspace, load_params


@dataclass
class VaeConfig:
    sample_size: int = 64                      # latent H = W
    in_channels: int = 4
    out_channels: int = 3
    block_out_channels: Tuple[int, ...] = (128, 256, 512, 512)
    layers_per_block: int = 2
    norm_num_groups: int = 32
    scaling_factor: float = 0.18215


def vae_param_shapes(cfg: VaeConfig) -> List[Tuple[str, Tuple[int, ...]]]:
    out: List[Tuple[str, Tuple[int, ...]]] = []
    add = lambda n, s: out.append((n, tuple(s)))
    nl = len(cfg.block_out_channels)
    top = cfg.block_out_channels[-1]

    def resnet(p, cin, cout):
        add(p + "norm1.weight", (cin,)); add(p + "norm1.bias", (cin,))
        add(p + "conv1.weight", (cout, cin, 3, 3)); add(p + "conv1.bias", (cout,))
        add(p + "norm2.weight", (cout,)); add(p + "norm2.bias", (cout,))
        add(p + "conv2.weight", (cout, cout, 3, 3)); add(p + "conv2.bias", (cout,))
        if cin != cout:
            add(p + "conv_shortcut.weight", (cout, cin, 1, 1)); add(p + "conv_shortcut.bias", (cout,))

    add("post_quant_conv.weight", (cfg.in_channels, cfg.in_channels, 1, 1)); add("post_quant_conv.bias", (cfg.in_channels,))
    add("decoder.conv_in.weight", (top, cfg.in_channels, 3, 3)); add("decoder.conv_in.bias", (top,))
    resnet("decoder.mid_block.resnets.0.", top, top)
    a = "decoder.mid_block.attentions.0."
    add(a + "group_norm.weight", (top,)); add(a + "group_norm.bias", (top,))
    for n in ("to_q", "to_k", "to_v", "to_out.0"):
        add(a + n + ".weight", (top, top)); add(a + n + ".bias", (top,))
    resnet("decoder.mid_block.resnets.1.", top, top)
    ch = top
    for i in range(nl):
        co = cfg.block_out_channels[nl - 1 - i]
        for j in range(cfg.layers_per_block + 1):
            resnet(f"decoder.up_blocks.{i}.resnets.{j}.", ch, co)
            ch = co
        if i < nl - 1:
            add(f"decoder.up_blocks.{i}.upsamplers.0.conv.weight", (co, co, 3, 3))
            add(f"decoder.up_blocks.{i}.upsamplers.0.conv.bias", (co,))
    add("decoder.conv_norm_out.weight", (ch,)); add("decoder.conv_norm_out.bias", (ch,))
    add("decoder.conv_out.weight", (cfg.out_channels, ch, 3, 3)); add("decoder.conv_out.bias", (cfg.out_channels,))
    return out


def vae_encoder_param_shapes(cfg: VaeConfig) -> List[Tuple[str, Tuple[int, ...]]]:
    """``encoder.*`` and ``quant_conv.*`` of diffusers' AutoencoderKL state dict, in module order."""
    out: List[Tuple[str, Tuple[int, ...]]] = []
    add = lambda n, s: out.append((n, tuple(s)))
    nl = len(cfg.block_out_channels)
    top, c0, zc = cfg.block_out_channels[-1], cfg.block_out_channels[0], 2 * cfg.in_channels

    def resnet(p, cin, cout):
        add(p + "norm1.weight", (cin,)); add(p + "norm1.bias", (cin,))
        add(p + "conv1.weight", (cout, cin, 3, 3)); add(p + "conv1.bias", (cout,))
        add(p + "norm2.weight", (cout,)); add(p + "norm2.bias", (cout,))
        add(p + "conv2.weight", (cout, cout, 3, 3)); add(p + "conv2.bias", (cout,))
        if cin != cout:
            add(p + "conv_shortcut.weight", (cout, cin, 1, 1)); add(p + "conv_shortcut.bias", (cout,))

    add("encoder.conv_in.weight", (c0, cfg.out_channels, 3, 3)); add("encoder.conv_in.bias", (c0,))
    ch = c0
    for i in range(nl):
        co = cfg.block_out_channels[i]
        for j in range(cfg.layers_per_block):
            resnet(f"encoder.down_blocks.{i}.resnets.{j}.", ch, co)
            ch = co
        if i < nl - 1:
            add(f"encoder.down_blocks.{i}.downsamplers.0.conv.weight", (co, co, 3, 3))
            add(f"encoder.down_blocks.{i}.downsamplers.0.conv.bias", (co,))
    resnet("encoder.mid_block.resnets.0.", top, top)
    a = "encoder.mid_block.attentions.0."
    add(a + "group_norm.weight", (top,)); add(a + "group_norm.bias", (top,))
    for n in ("to_q", "to_k", "to_v", "to_out.0"):
        add(a + n + ".weight", (top, top)); add(a + n + ".bias", (top,))
    resnet("encoder.mid_block.resnets.1.", top, top)
    add("encoder.conv_norm_out.weight", (top,)); add("encoder.conv_norm_out.bias", (top,))
    add("encoder.conv_out.weight", (zc, top, 3, 3)); add("encoder.conv_out.bias", (zc,))
    add("quant_conv.weight", (zc, zc, 1, 1)); add("quant_conv.bias", (zc,))
    return out


def _draw_synthetic(shapes, g) -> Dict[str, torch.Tensor]:
    sd = {}
    for name, shape in shapes:
        leaf = name.rsplit(".", 2)[-2]
        is_norm = "norm" in leaf
        if name.endswith(".bias"):
            t = torch.randn(shape, generator=g) * (0.1 if is_norm else 0.05)
        elif is_norm:
            t = 1.0 + 0.1 * torch.randn(shape, generator=g)
        else:
            t = torch.randn(shape, generator=g) / math.sqrt(math.prod(shape[1:]))
        sd[name] = t.to(torch.bfloat16).float()
    return sd


# The synthetic encoder's posterior: with the initialisation above the logvar half of the moments comes out around
# +0.2 +- 0.6 while the mean half has std ~0.47, i.e. an encoded image would be mostly posterior noise.  A trained VAE's
# posterior is narrow (SD-1.5: logvar around -17 .. -8), so the stand-in fixes the logvar biases of quant_conv at this
# constant: std = exp(0.5 * (-8 + 0.2)) ~ 0.02 next to a mean of std ~0.47.
SYNTHETIC_LOGVAR_BIAS = -8.0
_ENCODER_SEED_OFFSET = 7919          # the encoder tensors come from a generator of their own: seed + this


def make_synthetic_vae_state_dict(cfg: VaeConfig, seed: int = 4321) -> Dict[str, torch.Tensor]:
    """Seeded SD-1.5-shaped VAE weights on the bf16 grid (no VAE weights exist offline).  The decoder tensors are drawn
    first, from ``Generator(seed)`` alone; the encoder tensors from ``Generator(seed + 7919)``, so adding them moved no
    decoder value.  ``quant_conv.bias[latent channels:]`` (the logvar half) is ``SYNTHETIC_LOGVAR_BIAS``."""
    sd = _draw_synthetic(vae_param_shapes(cfg), torch.Generator().manual_seed(seed))
    enc = _draw_synthetic(vae_encoder_param_shapes(cfg), torch.Generator().manual_seed(seed + _ENCODER_SEED_OFFSET))
    enc["quant_conv.bias"][cfg.in_channels:] = SYNTHETIC_LOGVAR_BIAS
    sd.update(enc)
    return sd


def load_vae_state_dict(model_dir: str) -> Dict[str, torch.Tensor]:
    from safetensors.torch import load_file
    for cand in (os.path.join(model_dir, "vae", "diffusion_pytorch_model.safetensors"),
                 os.path.join(model_dir, "diffusion_pytorch_model.safetensors")):
        if os.path.isfile(cand):
            return {k: v.float() for k, v in load_file(cand).items()}
    raise FileNotFoundError(f"no local VAE weights under {model_dir!r}")


def _c_config(cfg: VaeConfig) -> _lib.SdUnetConfigFull:
    c = _lib.SdUnetConfigFull()
    c.sample_size, c.in_channels, c.out_channels = cfg.sample_size, cfg.in_channels, cfg.out_channels
    c.num_levels = len(cfg.block_out_channels)
    for i, v in enumerate(cfg.block_out_channels):
        c.block_out_channels[i] = v
    c.layers_per_block = cfg.layers_per_block
    c.norm_num_groups, c.norm_eps = cfg.norm_num_groups, 1e-6
    c.num_heads, c.cross_attention_dim, c.context_len = 1, 64, 1
    return c


class _VaeHandle(HipHandle):
    """What the four autoencoder halves share: the parameter loop with the legacy reshape, and one workspace per
    (batch, h, w) (exact key)."""

    def _load(self, shapes, state_dict: Dict[str, torch.Tensor]) -> None:
        load_params(self._lib, self._handle, shapes, state_dict, "VAE", reshape_legacy=True)
        self._finalize()

    def _reserve(self, batch: int, h: int, w: int) -> Workspace:
        if not self._wsp.holds((batch, h, w)):
            n = Workspace.bytes_or_raise(self._lib.sd_unet_workspace_bytes_hw(self._handle, batch, -1, h, w),
                                         "sd_unet_workspace_bytes_hw")
            self._wsp.reserve(n, (batch, h, w))
        return self._wsp

    def _workspace(self, batch: int, h: int, w: int) -> torch.Tensor:
        return self._reserve(batch, h, w).tensor


class HipVaeDecoder(_VaeHandle):
    """``vae.decode`` replacement: ``decoder(latents) -> [B,3,8h,8w]`` fp32 on the GPU."""

    def __init__(self, config: VaeConfig, state_dict: Dict[str, torch.Tensor], device: str = "cuda:0"):
        super().__init__(device)
        self.config = config
        torch.cuda.set_device(self.device)
        _lib.check(self._lib.sd_vae_create(C.byref(_c_config(config)), C.byref(self._handle)), "sd_vae_create")
        self._load(vae_param_shapes(config), state_dict)

    def decode(self, latents: torch.Tensor, latent_scale: float = 1.0, chunk: int = 8) -> torch.Tensor:
        """``latents * latent_scale`` -> decoded images (pass ``1 / scaling_factor`` to fuse the division
        of src/models.py:288).  Large batches are decoded ``chunk`` images at a time.  Latent sides: multiples of 8
        in [8, 128] (``sample_size`` is only the default); the images are ``[B, 3, 8h, 8w]``."""
        lat = latents.to(self.device, torch.float32).contiguous()
        if lat.dim() != 4 or lat.shape[1] != self.config.in_channels:
            raise ValueError(f"latents must be [B,{self.config.in_channels},h,w], got {tuple(lat.shape)}")
        b, c, h, w = lat.shape
        if not (8 <= h <= 128 and 8 <= w <= 128 and h % 8 == 0 and w % 8 == 0):
            raise ValueError(f"latents {h}x{w}: the VAE decoder takes sides that are multiples of 8 in [8, 128]")
        out = torch.empty((b, self.config.out_channels, 8 * h, 8 * w), dtype=torch.float32, device=self.device)
        for s in range(0, b, chunk):
            n = min(chunk, b - s)
            ws = self._reserve(n, h, w)
            _lib.check(self._lib.sd_vae_decode_hw(self._handle, _lib.current_stream(), lat[s:s + n].data_ptr(), n, h, w,
                                                  float(latent_scale), out[s:s + n].data_ptr(), ws.ptr, ws.nbytes),
                       "sd_vae_decode_hw")
        return out

    __call__ = decode


class HipVaeEncoder(_VaeHandle):
    """``vae.encode`` replacement: ``encode(images) -> moments [B, 8, H/8, W/8]`` (``[mean | logvar]``, fp32, on the GPU) and
    ``sample(moments)`` = ``DiagonalGaussianDistribution.sample() / .mode()`` times the scaling factor."""

    def __init__(self, config: VaeConfig, state_dict: Dict[str, torch.Tensor], device: str = "cuda:0"):
        super().__init__(device)
        self.config = config
        torch.cuda.set_device(self.device)
        _lib.check(self._lib.sd_vae_encoder_create(C.byref(_c_config(config)), C.byref(self._handle)), "sd_vae_encoder_create")
        self._load(vae_encoder_param_shapes(config), state_dict)

    def encode(self, images: torch.Tensor, chunk: int = 8) -> torch.Tensor:
        """``images`` [B, 3, H, W] in [0, 1] (the ``2x - 1`` of diffusers' VaeImageProcessor happens in the entry kernel) ->
        moments [B, 8, H/8, W/8].  H and W: multiples of 64 in [64, 1024] (latent sides that are multiples of 8 in [8, 128]).
        Large batches are encoded ``chunk`` images at a time."""
        img = images.to(self.device, torch.float32).contiguous()
        if img.dim() != 4 or img.shape[1] != self.config.out_channels:
            raise ValueError(f"images must be [B,{self.config.out_channels},H,W], got {tuple(img.shape)}")
        b, _, hh, ww = img.shape
        if hh % 64 or ww % 64 or not (64 <= hh <= 1024 and 64 <= ww <= 1024):
            raise ValueError(f"images {hh}x{ww}: the VAE encoder takes sides that are multiples of 64 in [64, 1024]")
        h, w = hh // 8, ww // 8
        out = torch.empty((b, 2 * self.config.in_channels, h, w), dtype=torch.float32, device=self.device)
        for s in range(0, b, chunk):
            n = min(chunk, b - s)
            ws = self._reserve(n, h, w)
            _lib.check(self._lib.sd_vae_encode_hw(self._handle, _lib.current_stream(), img[s:s + n].data_ptr(), n, h, w,
                                                  out[s:s + n].data_ptr(), ws.ptr, ws.nbytes), "sd_vae_encode_hw")
        return out

    def sample(self, moments: torch.Tensor, noise: Optional[torch.Tensor] = None, mode: str = "sample",
               scale: Optional[float] = None, generator=None) -> torch.Tensor:
        """``scale * (mean + exp(0.5 * clamp(logvar, -30, 20)) * noise)`` for ``mode="sample"`` (``noise`` drawn from
        ``generator`` on the host when not given), ``scale * mean`` for ``mode="argmax"``; ``scale`` defaults to the
        config's ``scaling_factor``.  One elementwise launch."""
        if mode not in ("sample", "argmax"):
            raise ValueError(f"mode={mode!r}: 'sample' or 'argmax'")
        m = moments.to(self.device, torch.float32).contiguous()
        zc = self.config.in_channels
        if m.dim() != 4 or m.shape[1] != 2 * zc:
            raise ValueError(f"moments must be [B,{2 * zc},h,w], got {tuple(m.shape)}")
        b, _, h, w = m.shape
        z = None
        if mode == "sample":
            if noise is None:
                noise = torch.randn((b, zc, h, w), generator=generator, dtype=torch.float32)
            if tuple(noise.shape) != (b, zc, h, w):
                raise ValueError(f"noise must be {(b, zc, h, w)}, got {tuple(noise.shape)}")
            z = noise.to(self.device, torch.float32).contiguous()
        out = torch.empty((b, zc, h, w), dtype=torch.float32, device=self.device)
        sc = self.config.scaling_factor if scale is None else float(scale)
        _lib.check(self._lib.sd_vae_posterior_sample(_lib.current_stream(), m.data_ptr(), _lib.ptr(z), float(sc),
                                                     out.data_ptr(), b, h * w), "sd_vae_posterior_sample")
        return out

    __call__ = encode


# ---- AutoencoderTiny (TAESD: diffusers 0.32 AutoencoderTiny / EncoderTiny / DecoderTiny / AutoencoderTinyBlock, upstream-recall) ----
# A 2.4 M-parameter all-convolutional autoencoder in the UNet's OWN scaled latent space (scaling_factor 1.0): no
# normalisation, no attention, every hidden conv 64 -> 64 channels.  DESIGN.md 4m; csrc/conv64.hip, csrc/taesd.hip.

@dataclass
class TinyVaeConfig:
    """The one structure that is built; ``check_tiny_vae_config`` refuses any other by the name of the field."""
    in_channels: int = 3
    out_channels: int = 3
    latent_channels: int = 4
    encoder_block_out_channels: Tuple[int, ...] = (64, 64, 64, 64)
    decoder_block_out_channels: Tuple[int, ...] = (64, 64, 64, 64)
    num_encoder_blocks: Tuple[int, ...] = (1, 3, 3, 3)
    num_decoder_blocks: Tuple[int, ...] = (3, 3, 3, 1)
    act_fn: str = "relu"
    upsample_fn: str = "nearest"
    scaling_factor: float = 1.0


# THE table of both halves, in module order: (kind, index in ``<half>.layers``).  csrc/taesd.hip holds the same table.
TINY_DECODER_LAYERS = (("entry", 0), ("block", 2), ("block", 3), ("block", 4), ("up", 6), ("block", 7), ("block", 8), ("block", 9),
                       ("up", 11), ("block", 12), ("block", 13), ("block", 14), ("up", 16), ("block", 17), ("exit", 18))
TINY_ENCODER_LAYERS = (("entry", 0), ("block", 1), ("down", 2), ("block", 3), ("block", 4), ("block", 5), ("down", 6), ("block", 7),
                       ("block", 8), ("block", 9), ("down", 10), ("block", 11), ("block", 12), ("block", 13), ("exit", 14))


def check_tiny_vae_config(cfg) -> TinyVaeConfig:
    """A ``TinyVaeConfig`` or the dict of a ``config.json`` -> the config, or ``NotImplementedError`` naming the field that
    differs from the structure the kernels are built for."""
    want = TinyVaeConfig()
    if isinstance(cfg, TinyVaeConfig):
        cfg = dataclasses.asdict(cfg)
    for f in dataclasses.fields(TinyVaeConfig):
        if f.name not in cfg:
            continue
        got, exp = cfg[f.name], getattr(want, f.name)
        if isinstance(exp, tuple):
            got = tuple(got)
        if got != exp:
            raise NotImplementedError(f"AutoencoderTiny with {f.name}={cfg[f.name]!r} is not built ({f.name}={list(exp) if isinstance(exp, tuple) else exp!r} "
                                      "is: 64-channel blocks, encoder 1,3,3,3 / decoder 3,3,3,1, relu, nearest, 4 latent channels)")
    return want


def _tiny_half_shapes(half: str, layers, cin: int, cout: int) -> List[Tuple[str, Tuple[int, ...]]]:
    out: List[Tuple[str, Tuple[int, ...]]] = []
    for kind, n in layers:
        p = f"{half}.layers.{n}."
        if kind == "entry":
            out += [(p + "weight", (64, cin, 3, 3)), (p + "bias", (64,))]
        elif kind == "block":
            for k in (0, 2, 4):
                out += [(f"{p}conv.{k}.weight", (64, 64, 3, 3)), (f"{p}conv.{k}.bias", (64,))]
        elif kind == "exit":
            out += [(p + "weight", (cout, 64, 3, 3)), (p + "bias", (cout,))]
        else:                        # the convs behind an upsample / the stride-2 convs: no bias
            out += [(p + "weight", (64, 64, 3, 3))]
    return out


def tiny_vae_decoder_param_shapes(cfg: Optional[TinyVaeConfig] = None):
    return _tiny_half_shapes("decoder", TINY_DECODER_LAYERS, 4, 3)


def tiny_vae_encoder_param_shapes(cfg: Optional[TinyVaeConfig] = None):
    return _tiny_half_shapes("encoder", TINY_ENCODER_LAYERS, 3, 4)


def tiny_vae_param_shapes(cfg: Optional[TinyVaeConfig] = None) -> List[Tuple[str, Tuple[int, ...]]]:
    """diffusers' AutoencoderTiny state dict: 134 tensors, 2,445,063 values (encoder first, as the module registers them)."""
    if cfg is not None:
        check_tiny_vae_config(cfg)
    return tiny_vae_encoder_param_shapes() + tiny_vae_decoder_param_shapes()


TINY_SYNTHETIC_SEED = 4
TINY_EXIT_IMAGE_FACTOR = 0.1        # the stand-in's 64 -> 3 exit: N(0, 1 / fan_in) x this, bias 0.5 + 0.05 N


def make_synthetic_tiny_vae_state_dict(cfg: Optional[TinyVaeConfig] = None, seed: Optional[int] = None) -> Dict[str, torch.Tensor]:
    """Seeded stand-in for a hub AutoencoderTiny, on the bf16 grid (no such weights exist offline).  Conv weights are
    N(0, 2 / fan_in) (ReLU networks keep their activation scale with it), each block's last conv (``conv.4``) x 0.5 so that
    the residual sums stay bounded through 10 blocks, the 64 -> 4 exit N(0, 1 / fan_in); the 64 -> 3 exit N(0, 1 / fan_in) x
    ``TINY_EXIT_IMAGE_FACTOR`` with bias 0.5 + 0.05 N, which puts the picture around mid-grey with few clamped pixels; every
    other bias 0.05 N.  Drawn in the order of ``tiny_vae_param_shapes``.  The picture's spread depends on the seed (the
    residual stream's scale after 10 blocks does): at the default seed the decoded picture has std 0.16 .. 0.19 with under 1 %
    of its pixels clamped (tests/test_taesd_cpu.py holds it to std >= 0.1 and < 2 %)."""
    if cfg is not None:
        check_tiny_vae_config(cfg)
    if seed is None:
        seed = TINY_SYNTHETIC_SEED
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for name, shape in tiny_vae_param_shapes():
        if name.endswith(".bias"):
            t = 0.05 * torch.randn(shape, generator=g)
            if name == "decoder.layers.18.bias":
                t = t + 0.5
        else:
            fan_in = math.prod(shape[1:])
            t = torch.randn(shape, generator=g) * math.sqrt(2.0 / fan_in)
            if name.endswith("conv.4.weight"):
                t = t * 0.5
            elif name == "encoder.layers.14.weight":
                t = t * math.sqrt(0.5)
            elif name == "decoder.layers.18.weight":
                t = t * math.sqrt(0.5) * TINY_EXIT_IMAGE_FACTOR
        sd[name] = t.to(torch.bfloat16).float()
    return sd


def load_tiny_vae_state_dict(model_dir: str) -> Dict[str, torch.Tensor]:
    """A LOCAL AutoencoderTiny directory (``config.json`` + ``diffusion_pytorch_model.safetensors``).  The config must be
    the structure that is built (``check_tiny_vae_config``); key names and shapes are checked strictly, both ways."""
    import json
    from safetensors.torch import load_file
    cfg_path = os.path.join(model_dir, "config.json")
    w_path = os.path.join(model_dir, "diffusion_pytorch_model.safetensors")
    if not os.path.isfile(cfg_path) or not os.path.isfile(w_path):
        raise FileNotFoundError(f"no local AutoencoderTiny under {model_dir!r} (config.json + diffusion_pytorch_model.safetensors)")
    check_tiny_vae_config(json.load(open(cfg_path)))
    sd = {k: v.float() for k, v in load_file(w_path).items()}
    shapes = dict(tiny_vae_param_shapes())
    missing, extra = sorted(set(shapes) - set(sd)), sorted(set(sd) - set(shapes))
    if missing or extra:
        raise KeyError(f"AutoencoderTiny state dict: missing {missing[:4]}{'...' if len(missing) > 4 else ''}, "
                       f"unexpected {extra[:4]}{'...' if len(extra) > 4 else ''}")
    for k, s in shapes.items():
        if tuple(sd[k].shape) != s:
            raise ValueError(f"{k}: expected shape {s}, got {tuple(sd[k].shape)}")
    return sd


class _HipTinyHalf(_VaeHandle):
    _create = ""
    _shapes = staticmethod(lambda: [])

    def __init__(self, state_dict: Dict[str, torch.Tensor], config: Optional[TinyVaeConfig] = None, device: str = "cuda:0"):
        super().__init__(device)
        self.config = check_tiny_vae_config(config or TinyVaeConfig())
        torch.cuda.set_device(self.device)
        _lib.check(getattr(self._lib, self._create)(C.byref(self._handle)), self._create)
        self._load(self._shapes(), state_dict)


class HipTinyVaeDecoder(_HipTinyHalf):
    """``AutoencoderTiny.decode`` on libsdhip: UNet latents AS THEY ARE (scaling_factor 1.0) -> images, 35 launches."""
    _create = "sd_taesd_decoder_create"
    _shapes = staticmethod(tiny_vae_decoder_param_shapes)

    def decode(self, latents: torch.Tensor, unit_range: bool = False, chunk: int = 8) -> torch.Tensor:
        """[B,4,h,w] -> [B,3,8h,8w] fp32 on the GPU: in [-1, 1] as diffusers returns it (``y * 2 - 1``), or with
        ``unit_range`` the picture itself clamped to [0, 1] (what ``/ 2 + 0.5`` and ``clamp`` make of the former, without
        those two passes).  Latent sides: multiples of 8 in [8, 128]; ``chunk`` images per call of the library."""
        lat = latents.to(self.device, torch.float32).contiguous()
        if lat.dim() != 4 or lat.shape[1] != 4:
            raise ValueError(f"latents must be [B,4,h,w], got {tuple(lat.shape)}")
        b, _, h, w = lat.shape
        if not (8 <= h <= 128 and 8 <= w <= 128 and h % 8 == 0 and w % 8 == 0):
            raise ValueError(f"latents {h}x{w}: the tiny decoder takes sides that are multiples of 8 in [8, 128]")
        out = torch.empty((b, 3, 8 * h, 8 * w), dtype=torch.float32, device=self.device)
        for s in range(0, b, chunk):
            n = min(chunk, b - s)
            ws = self._reserve(n, h, w)
            _lib.check(self._lib.sd_taesd_decode_hw(self._handle, _lib.current_stream(), lat[s:s + n].data_ptr(), n, h, w,
                                                    1 if unit_range else 0, out[s:s + n].data_ptr(), ws.ptr, ws.nbytes),
                       "sd_taesd_decode_hw")
        return out

    __call__ = decode


class HipTinyVaeEncoder(_HipTinyHalf):
    """``AutoencoderTiny.encode(...).latents`` on libsdhip: images in [0, 1] -> latents in the UNet's scaled space."""
    _create = "sd_taesd_encoder_create"
    _shapes = staticmethod(tiny_vae_encoder_param_shapes)

    def encode(self, images01: torch.Tensor, chunk: int = 8) -> torch.Tensor:
        """[B,3,H,W] in [0, 1] -> [B,4,H/8,W/8] fp32 on the GPU (no posterior, nothing is drawn).  H and W: multiples of 64
        in [64, 1024]."""
        img = images01.to(self.device, torch.float32).contiguous()
        if img.dim() != 4 or img.shape[1] != 3:
            raise ValueError(f"images must be [B,3,H,W], got {tuple(img.shape)}")
        b, _, hh, ww = img.shape
        if hh % 64 or ww % 64 or not (64 <= hh <= 1024 and 64 <= ww <= 1024):
            raise ValueError(f"images {hh}x{ww}: the tiny encoder takes sides that are multiples of 64 in [64, 1024]")
        h, w = hh // 8, ww // 8
        out = torch.empty((b, 4, h, w), dtype=torch.float32, device=self.device)
        for s in range(0, b, chunk):
            n = min(chunk, b - s)
            ws = self._reserve(n, h, w)
            _lib.check(self._lib.sd_taesd_encode_hw(self._handle, _lib.current_stream(), img[s:s + n].data_ptr(), n, h, w,
                                                    out[s:s + n].data_ptr(), ws.ptr, ws.nbytes), "sd_taesd_encode_hw")
        return out

    __call__ = encode
