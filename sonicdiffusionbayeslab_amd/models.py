"""``StableDiffusionModel`` -- the reference's pipeline plugin over the MI355X-native kernels.

Registered as ``models_registry["stable_diffusion_model"]`` like ``src/models.py:21`` of the
reference and callable the same way (``src/models.py:23-29,32-335``):

    images, execution_time, x0_preds = model(prompts, num_inference_steps=N, guidance_scale=7.5,
                                             generator=g, output_type="pt")

The denoising loop (``src/models.py:210-282``) is restated with three changes that are the
point of this framework: the UNet forward is libsdhip (hand-written gfx950 kernels), the CFG
duplication is fused into conv_in, and CFG-combine + ``scheduler.step`` is one fused launch.
Timing keeps the reference's definition -- wall-clock of the loop only (``:208,284-285``) -- but
brackets it with device synchronisation so the number is real.

``output_type="pt"`` decodes through the libsdhip AutoencoderKL decoder (``vae.py``, SURVEY 8f row 1;
outside the timed loop, as in the reference).  The three variant pipelines of ``src/models.py:338-1467``
(two schedulers, interleaved schedulers, skipped timesteps) are host-only control flow over
the same kernels and live at the bottom of this file.  Prompts are encoded by a pluggable ``text_encoder``:
the CLIP text tower on libsdhip + BPE tokenizer (``clip.py``) when the checkpoint directory
carries ``tokenizer/`` and ``text_encoder/``, otherwise a deterministic seeded stand-in (no CLIP weights
exist offline) -- ``weights_source`` / the reports say which.
"""
from __future__ import annotations

import hashlib
import math
import os
import time
from dataclasses import dataclass
from types import SimpleNamespace
from typing import Callable, List, Optional, Union

import torch

from . import dist as sdist
from . import options
from .registry import models_registry
from .schedulers import PNDMConfigStub, pag_step_scale, sag_degrade
from .unet import CACHE_FULL_AND_STORE, CACHE_OFF, CACHE_SKIP, LATENT_CHANNELS, HipUNet2DConditionModel
from .vae import HipVaeDecoder, HipVaeEncoder, VaeConfig, load_vae_state_dict, make_synthetic_vae_state_dict
from .weights import (SD2_CONTEXT_DIM, SD2_HEADS, UNetConfig, check_projection_layout, load_scheduler_config, load_unet_config,
                      load_unet_state_dict, make_synthetic_state_dict, sd2_unet_config)


@dataclass
class StableDiffusionPipelineOutput:
    images: torch.Tensor
    nsfw_content_detected: Optional[list] = None


class SyntheticTextEncoder:
    """Deterministic stand-in for CLIP ViT-L/14 text encoding: a prompt's [77,768] embedding is
    drawn ~N(0,1) from a generator seeded by the prompt's SHA-256.  Same prompt -> same
    embedding on every rank and box; documented as synthetic in every report."""

    def __init__(self, context_len: int = 77, dim: int = 768):
        self.context_len, self.dim = context_len, dim
        self._cache = {}

    def __call__(self, prompts: List[str]) -> torch.Tensor:
        out = []
        for p in prompts:
            if p not in self._cache:
                seed = int.from_bytes(hashlib.sha256(p.encode("utf-8")).digest()[:8], "little") & (2 ** 63 - 1)
                g = torch.Generator().manual_seed(seed)
                self._cache[p] = torch.randn((self.context_len, self.dim), generator=g)
            out.append(self._cache[p])
        return torch.stack(out)


class _VaeConfig:
    scaling_factor = 0.18215


class _Unset:
    """Default of ``strength``: 0.8 for image-to-image, 1.0 with ``mask_image`` (upstream's defaults); an explicit value wins."""

    def __repr__(self):
        return "<0.8, or 1.0 with mask_image>"


STRENGTH_UNSET = _Unset()


def get_guidance_scale_embedding(w, embedding_dim: int = 512, dtype=torch.float32) -> torch.Tensor:
    """Guidance-scale embedding of LCM-distilled UNets (diffusers ``LatentConsistencyModelPipeline``; the reference feeds
    ``w = guidance_scale - 1``, ``src/models.py:195-202``): ``w`` (scalar or [n]) -> [n, embedding_dim] =
    ``[sin(1000 w f_k) | cos(1000 w f_k)]``, ``f_k = exp(-k ln(10000) / (half - 1))``, one zero column appended for an odd
    dimension.  Not the timestep sinusoid (that one is ``[cos | sin]`` with denominator ``half``)."""
    w = torch.as_tensor(w, dtype=torch.float32).reshape(-1) * 1000.0
    half = embedding_dim // 2
    freq = torch.exp(torch.arange(half, dtype=dtype) * -(math.log(10000.0) / (half - 1)))
    emb = w.to(dtype)[:, None] * freq[None, :]
    emb = torch.cat([torch.sin(emb), torch.cos(emb)], dim=1)
    if embedding_dim % 2 == 1:
        emb = torch.nn.functional.pad(emb, (0, 1))
    return emb


def postprocess_images(image01: torch.Tensor, output_type: str):
    """The tail of ``src/models.py:312-321`` (diffusers ``VaeImageProcessor.postprocess`` on denormalised images):
    ``image01`` is ``[B, 3, H, W]`` in [0, 1].  "pt": as is; "np": float32 ``[B, H, W, 3]`` on the host; "pil": a list of
    ``PIL.Image`` (uint8, ``round(255 x)``)."""
    if output_type == "pt":
        return image01
    arr = image01.detach().to("cpu", torch.float32).permute(0, 2, 3, 1).contiguous().numpy()
    if output_type == "np":
        return arr
    if output_type == "pil":
        from PIL import Image
        return [Image.fromarray(a) for a in (arr * 255.0).round().astype("uint8")]
    raise NotImplementedError(f"output_type {output_type!r}")


def _prompt_batch(prompt, prompt_embeds) -> int:
    """The number of prompts of a call: one string, a list of them, or the rows of ``prompt_embeds``."""
    if prompt is None:
        return int(prompt_embeds.shape[0])
    return 1 if isinstance(prompt, str) else len(prompt)


def _is_pil_list(v) -> bool:
    return isinstance(v, (list, tuple)) and len(v) > 0 and all(hasattr(im, "convert") for im in v)


def _pil_stack(images, mode: str, dtype, what: str):
    """A list of PIL images of one size -> one numpy array [B, H, W(, 3)] of ``dtype`` in ``mode`` ("RGB" | "L").
    ``what`` names the argument in the refusal of mixed sizes."""
    import numpy as np
    sizes = {im.size for im in images}
    if len(sizes) != 1:
        raise ValueError(f"{what} of one call must have one size, got {sorted(sizes)}")
    return np.stack([np.asarray(im.convert(mode), dtype=dtype) for im in images])


@models_registry.add_to_registry("stable_diffusion_model")
class StableDiffusionModel:
    vae_scale_factor = 8

    def __init__(self, unet_config: Optional[UNetConfig] = None, state_dict=None, scheduler=None,
                 text_encoder: Optional[Callable] = None, vae_decoder: Optional[Callable] = None,
                 weights_seed: int = 1234, source: str = "synthetic", clip_dir: Optional[str] = None,
                 weight_dtype: Optional[str] = None):
        self.unet_config = unet_config or UNetConfig()
        # "bf16" | "fp8": operand type of the UNet's MFMA contractions (YAML model.weight_dtype, or SD_AMD_WEIGHT_DTYPE)
        self.weight_dtype = weight_dtype or os.environ.get("SD_AMD_WEIGHT_DTYPE", "bf16")
        self._state_dict = state_dict
        self._weights_seed = weights_seed
        self.weights_source = source
        self.unet: Optional[HipUNet2DConditionModel] = None
        self.scheduler = scheduler or PNDMConfigStub()
        self.text_encoder = text_encoder or SyntheticTextEncoder(self.unet_config.context_len,
                                                                 self.unet_config.cross_attention_dim)
        # a local checkpoint with tokenizer/ + text_encoder/: the CLIP text tower on libsdhip replaces the stand-in
        self._clip_dir = clip_dir if text_encoder is None else None
        self.vae_decoder = vae_decoder
        self.vae_encoder = None         # HipVaeEncoder, built by the first image-to-image call
        self.vae_config = _VaeConfig()
        self.device = torch.device("cpu")
        self._num_timesteps = 0
        self._guidance_scale = 7.5
        self._deepcache = None          # set by DeepCacheSDHelper.enable()
        self._lora = []
        self._fp8_calibrated = False    # fp8 handles: per-tensor activation scales, calibrated once on a FIXED seeded batch
        self._size = None               # (height, width) in pixels of the current call, set by _begin
        self.fp8_scales = {}            # {tensor name: scale} in use (reported by the harness next to the results)
        # IP-Adapter (load_ip_adapter): its UNet-named weights until the handle is built, the scale of the image branch, the
        # local image_encoder directory (ip_adapter_image) and its tower, and the embeds of the call in progress
        self._ip_sd = None
        self._ip_loaded = False
        self._ip_source = None          # what load_ip_adapter appended to weights_source (unload_ip_adapter takes it off)
        self._ip_scale = 1.0
        self._ip_encoder_dir = None
        self._ip_encoder = None
        self._ip_pending = None
        # ControlNet (load_controlnet): its config and weights (or the seed of a hub name's stand-in) until the handle is
        # built, the handle, the checked arguments of the call in progress and what its loop runs with
        self._cn_cfg = None
        self._cn_sd = None
        self._cn_seed = None
        self._cn_source = None
        self.controlnet = None
        self._cn_run = None
        self.control_image = None       # the control image of the last conditioned call, at the call's size
        # AutoencoderTiny (load_tiny_vae): its weights (or the seed of a hub name's stand-in) until the handles are built,
        # what it is used for ("all" | "previews" | None = not loaded) and the two handles
        self._tiny_sd = None
        self._tiny_seed = None
        self._tiny_source = None
        self.tiny_vae_use = None
        self.tiny_vae_decoder = None
        self.tiny_vae_encoder = None
        # Token Merging (apply_tome): dict(ratio, max_downsample, use_rand, seed, rand_every) or None = off; the generator of
        # the dst choices and the cell count of the call in progress
        self._tome = None
        self._tome_gen = None
        self._tome_cells = 0
        self._tome_first = False        # the call's first forward uses the choice array _tome_begin uploaded
        self._freeu = None              # FreeU (enable_freeu): (s1, s2, b1, b2) or None = off
        self._hypertile = None          # HyperTile (enable_hypertile): (tile_tokens, max_depth) or None = off
        self._tgate_step = None         # T-GATE (enable_tgate): the gate step, or None = off
        self._pag = None                # PAG (enable_pag): dict(scale, adaptive_scale, layers, mask) or None = off
        self._pag_call = None           # the running call's (pag_scale, pag_adaptive_scale), None = a plain call
        self._sag = None                # SAG (enable_sag): the default sag_scale, or None = off
        self._sag_call = None           # the running call's sag_scale, None = a plain call
        self._sag_keep = False          # keep the per-step attention masses of a call in sag_masses ([LB, mh, mw] fp32 each)
        self.sag_masses = []
        self._tgate_reserved = False    # the UNet's workspaces are sized for the capture plans as well

    # -- options and the pairs of them that are not built (options.py) -------------------
    IS_VARIANT = False              # the variant pipelines: options.VARIANT is on

    @classmethod
    def _model_options(cls, unet_config, weight_dtype) -> list:
        """What a model has on by construction: its pipeline class and its UNet's dtype, input channels and adapter weights."""
        return ([options.VARIANT] if cls.IS_VARIANT else []) + options.handle_options(unet_config, weight_dtype)

    def _enabled(self, among=options.OPTIONS) -> list:
        """The options ``enable_*`` / ``apply_tome`` / the DeepCache helper have switched on, of those in ``among``."""
        state = ((options.DEEPCACHE, self._deepcache is not None), (options.TOME, self._tome is not None),
                 (options.HYPERTILE, self._hypertile is not None), (options.FREEU, self._freeu is not None),
                 (options.TGATE, self._tgate_step is not None))
        return [name for name, on in state if on and name in among]

    def _call_options(self, control=None, ip_adapter_image=None, ip_adapter_image_embeds=None, guidance_rescale=None) -> list:
        """Everything one call runs with beside the option it checks: the model's own, what is enabled, a ControlNet or an
        IP-Adapter loaded or passed, PAG when this call runs it, ``guidance_rescale``."""
        state = ((options.CONTROL, control is not None or getattr(self, "_cn_cfg", None) is not None),
                 (options.IP_PROMPT, ip_adapter_image is not None or ip_adapter_image_embeds is not None or self._ip_loaded),
                 (options.PAG, self._pag_call is not None),
                 (options.RESCALE, guidance_rescale is not None and guidance_rescale > 0.0))
        return self._model_options(self.unet_config, self.weight_dtype) + self._enabled() + [name for name, on in state if on]

    # -- Token Merging (tomesd.apply_patch) ----------------------------------------------------------
    TOME_MAX_RATIO = 0.75

    @staticmethod
    def check_tome_args(ratio=0.5, max_downsample=1, sx=2, sy=2, use_rand=True, merge_attn=True, merge_crossattn=False,
                        merge_mlp=False, seed=0, rand_every="step", weight_dtype="bf16"):
        """The arguments of ``apply_tome`` checked, by name, without touching the GPU.  Returns the setting as a dict, or
        None for ``ratio == 0`` (off)."""
        if isinstance(ratio, bool) or not isinstance(ratio, (int, float)) or not 0.0 <= float(ratio) <= StableDiffusionModel.TOME_MAX_RATIO:
            raise ValueError(f"ratio={ratio!r}: Token Merging takes a ratio in [0, {StableDiffusionModel.TOME_MAX_RATIO}] "
                             "(a 2x2 cell has three src tokens)")
        if sx != 2 or sy != 2:
            raise NotImplementedError(f"sx={sx!r}, sy={sy!r}: only 2x2 cells are built")
        if max_downsample not in (1, 2):
            raise NotImplementedError(f"max_downsample={max_downsample!r}: 1 (the first level) or 2 (the first two) are built")
        if not merge_attn:
            raise NotImplementedError("merge_attn=False: merging around the self-attention is the only form built")
        if merge_crossattn:
            raise NotImplementedError("merge_crossattn=True: merging around the cross-attention is not built")
        if merge_mlp:
            raise NotImplementedError("merge_mlp=True: merging around the feed-forward is not built")
        if rand_every not in ("step", "call"):
            raise ValueError(f"rand_every={rand_every!r}: 'step' (a fresh dst choice before every UNet forward) or 'call'")
        if float(ratio) > 0.0:
            options.check(options.TOME, options.handle_options(None, weight_dtype))
        if float(ratio) == 0.0:
            return None
        return dict(ratio=float(ratio), max_downsample=int(max_downsample), use_rand=bool(use_rand), seed=int(seed),
                    rand_every=rand_every)

    def apply_tome(self, ratio: float = 0.5, max_downsample: int = 1, sx: int = 2, sy: int = 2, use_rand: bool = True,
                   merge_attn: bool = True, merge_crossattn: bool = False, merge_mlp: bool = False, seed: int = 0,
                   rand_every: str = "step"):
        """Token Merging for Stable Diffusion (``tomesd.apply_patch``): every later call merges
        ``min(num_src, int(tokens * ratio))`` tokens around the self-attention of the transformer blocks at the first
        ``max_downsample`` levels.  The dst token of each 2x2 cell is drawn on the host with ``torch.randint`` from a CPU
        generator seeded by ``seed`` at the start of a call -- before every UNet forward (``rand_every="step"``) or once per call
        (``"call"``); ``use_rand=False`` takes the top-left token of every cell.  ``ratio=0`` is ``remove_tome()``."""
        new = self.check_tome_args(ratio, max_downsample, sx, sy, use_rand, merge_attn, merge_crossattn, merge_mlp, seed,
                                   rand_every, self.weight_dtype)
        if new is not None:
            options.check(options.TOME, self._enabled({options.HYPERTILE}))
        self._tome = new
        return self

    def remove_tome(self):
        """Later calls are those of a model that never saw Token Merging, bit for bit."""
        self._tome = None
        return self

    @staticmethod
    def draw_tome_choice(generator: torch.Generator, cells: int) -> torch.Tensor:
        """The dst positions (0..3) of all merging blocks of one forward: one draw, whatever the rank or world size."""
        return torch.randint(4, (cells,), generator=generator, dtype=torch.uint8)

    def _tome_upload(self):
        choice = self.draw_tome_choice(self._tome_gen, self._tome_cells) if self._tome["use_rand"] else \
            torch.zeros(self._tome_cells, dtype=torch.uint8)
        self.unet.set_tome_choice(choice.pin_memory().to(self.unet.device, non_blocking=True), *self.latent_size)

    def _tome_begin(self):
        """Start of a sampling loop: the setting onto the UNet handle, a fresh generator, the call's first choice array."""
        t = self._tome
        self._tome_gen = None
        if t is None:
            self.unet.set_tome(0.0)
            return
        self.unet.set_tome(t["ratio"], t["max_downsample"])
        blocks = self.unet.tome_blocks(*self.latent_size)
        self._tome_cells = sum((b["h"] // 2) * (b["w"] // 2) for b in blocks)
        self._tome_gen = torch.Generator().manual_seed(t["seed"])
        if self._tome_cells:
            self._tome_upload()
        self._tome_first = True

    def _tome_step(self):
        """Before every UNet forward: ``rand_every="step"`` uploads a fresh dst choice (the first forward uses the one
        ``_tome_begin`` drew)."""
        t = self._tome
        if t is None or self._tome_gen is None or not self._tome_cells:
            return
        if self._tome_first:
            self._tome_first = False
            return
        if t["use_rand"] and t["rand_every"] == "step":
            self._tome_upload()

    # -- HyperTile (tfernd/HyperTile) ------------------------------------------------------
    @staticmethod
    def check_hypertile_args(tile_size=256, max_depth=0, swap_size=1, weight_dtype="bf16"):
        """The arguments of ``enable_hypertile`` checked, by name, without touching the GPU.  Returns ``(tile_tokens,
        max_depth)``: the tile side in tokens is ``tile_size // 8``."""
        if isinstance(tile_size, bool) or not isinstance(tile_size, int) or tile_size % 8 != 0 or not 64 <= tile_size <= 2048:
            raise ValueError(f"tile_size={tile_size!r}: HyperTile takes a tile size in pixels that is a multiple of 8, "
                             "at least 64 and at most 2048")
        if isinstance(max_depth, bool) or not isinstance(max_depth, int) or not 0 <= max_depth <= 3:
            raise ValueError(f"max_depth={max_depth!r}: HyperTile takes an integer max_depth of 0 .. 3")
        if isinstance(swap_size, bool) or swap_size != 1:
            raise NotImplementedError(f"swap_size={swap_size!r}: only swap_size=1 is built (upstream's per-step random choice "
                                      "among several tile sizes is not)")
        return HipUNet2DConditionModel.check_hypertile_args(tile_size // 8, max_depth, weight_dtype)

    def enable_hypertile(self, tile_size: int = 256, max_depth: int = 0, swap_size: int = 1):
        """HyperTile: in every later call the transformer blocks at depth ``<= max_depth`` (0 = the latent's own level) run
        their self-attention inside tiles of about ``tile_size`` pixels: the tile side in tokens is the smallest divisor of
        the level's side that is ``>= tile_size // 8``; a level that the rule leaves in one tile is not tiled.  Valid with
        every pipeline and scheduler, DeepCache, T-GATE, FreeU, LCM-distilled UNets, SD 2.x, IP-Adapter, ControlNet, TAESD,
        every image size and batch sharding; refused by name with Token Merging and on fp8 UNets."""
        new = self.check_hypertile_args(tile_size, max_depth, swap_size, self.weight_dtype)
        options.check(options.HYPERTILE, self._enabled({options.TOME}))
        self._hypertile = new
        return self

    def disable_hypertile(self):
        """Later calls are those of a model that never saw HyperTile, bit for bit."""
        self._hypertile = None
        return self

    def _hypertile_begin(self):
        """Start of a sampling loop: the setting onto the UNet handle.  A handle that never had the setting on is not touched
        while it is off."""
        if self._hypertile is not None:
            self.unet.set_hypertile(*self._hypertile)
        elif getattr(self.unet, "_hypertile", None) is not None:
            self.unet.set_hypertile(0)

    # -- perturbed-attention guidance (diffusers PAGMixin) -----------------------------------
    @staticmethod
    def check_pag_scales(pag_scale, pag_adaptive_scale):
        """``pag_scale`` / ``pag_adaptive_scale`` of ``enable_pag`` or of a call: finite numbers, the adaptive scale >= 0
        (``ValueError`` otherwise).  Returns them as floats."""
        out = []
        for name, v in (("pag_scale", pag_scale), ("pag_adaptive_scale", pag_adaptive_scale)):
            if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(float(v)):
                raise ValueError(f"{name}={v!r}: a finite number (pag_scale <= 0 is the plain pipeline)")
            out.append(float(v))
        if out[1] < 0.0:
            raise ValueError(f"pag_adaptive_scale={pag_adaptive_scale!r}: must be >= 0 (the scale falls by it per timestep below 1000)")
        return out[0], out[1]

    @classmethod
    def check_pag_args(cls, pag_scale=3.0, pag_adaptive_scale=0.0, pag_applied_layers="mid", unet_config=None,
                       weight_dtype="bf16"):
        """Everything ``enable_pag`` can refuse from the model alone, by name, without touching the GPU.  Returns the setting:
        dict(scale, adaptive_scale, layers, mask) -- ``mask`` is None without a ``unet_config`` to resolve the names against."""
        scale, adaptive = cls.check_pag_scales(pag_scale, pag_adaptive_scale)
        options.check(options.PAG, cls._model_options(unet_config, weight_dtype))
        layers = [pag_applied_layers] if isinstance(pag_applied_layers, str) else list(pag_applied_layers)
        mask = None
        if unet_config is not None:
            mask = HipUNet2DConditionModel.pag_layer_mask(unet_config, layers)
        return dict(scale=scale, adaptive_scale=adaptive, layers=layers, mask=mask)

    def enable_pag(self, pag_scale: float = 3.0, pag_adaptive_scale: float = 0.0, pag_applied_layers="mid"):
        """Perturbed-attention guidance (Ahn et al. 2024; diffusers' ``StableDiffusionPAGPipeline``): every later call runs a
        third UNet branch -- the conditional one with the self-attention of the transformer blocks ``pag_applied_layers``
        names (``"mid"``, ``"down.block_i"``, ``"up.block_i"``, ``"...attentions_j"``, or a list) replaced by the identity --
        and the step adds ``s_t * (cond - perturbed)`` to the guided prediction, ``s_t = pag_scale`` or, with
        ``pag_adaptive_scale > 0``, ``max(pag_scale - pag_adaptive_scale * (1000 - t), 0)``.  Works with and without CFG (an
        LCM-distilled UNet runs [cond | perturbed]).  ``pag_scale`` / ``pag_adaptive_scale`` given to a call override these
        defaults; ``pag_scale <= 0`` is the plain pipeline, bit for bit.  Valid with text-to-image, image-to-image and
        4-channel inpainting, every scheduler, ``guidance_rescale``, SD 2.x, HyperTile, FreeU, TAESD, every image size and
        batch sharding; refused by name with Token Merging, T-GATE, DeepCache, IP-Adapter, ControlNet, 9-channel
        inpainting UNets, fp8 and on the variant pipelines."""
        self._pag = self.check_pag_args(pag_scale, pag_adaptive_scale, pag_applied_layers, self.unet_config, self.weight_dtype)
        return self

    def disable_pag(self):
        """Later calls are those of a model that never saw PAG, bit for bit."""
        self._pag = None
        return self

    def _pag_check_call(self, pag_scale, pag_adaptive_scale, control=None, ip_adapter_image=None, ip_adapter_image_embeds=None):
        """The PAG setting of one call -- ``(pag_scale, pag_adaptive_scale)``, the call's own values over ``enable_pag``'s, or None
        for a plain call (PAG off, or ``pag_scale <= 0``) -- and what a PAG call refuses, by name, before any GPU work."""
        if self._pag is None:
            if pag_scale is not None or pag_adaptive_scale is not None:
                raise ValueError("pag_scale / pag_adaptive_scale given, but PAG is off: enable_pag(pag_applied_layers=...) first "
                                 "(the perturbed layers are part of the UNet's plans)")
            return None
        scale, adaptive = self.check_pag_scales(self._pag["scale"] if pag_scale is None else pag_scale,
                                                self._pag["adaptive_scale"] if pag_adaptive_scale is None else pag_adaptive_scale)
        if scale <= 0.0:
            return None
        self.check_pag_args(scale, adaptive, self._pag["layers"], self.unet_config, self.weight_dtype)
        options.check(options.PAG, self._call_options(control, ip_adapter_image, ip_adapter_image_embeds))
        return scale, adaptive

    def _pag_begin(self):
        """Start of a sampling loop: the layer mask onto the UNet handle, or off it.  A handle that never had one is not touched
        while PAG is off."""
        if self._pag_call is not None:
            self.unet.set_pag(self._pag["mask"])
        elif getattr(self.unet, "_pag", 0):
            self.unet.set_pag(0)

    # -- self-attention guidance (diffusers StableDiffusionSAGPipeline) -------------------------
    @staticmethod
    def check_sag_scale(sag_scale):
        """``sag_scale`` of ``enable_sag`` or of a call: a finite number (``ValueError`` otherwise).  Returns it as a float."""
        if isinstance(sag_scale, bool) or not isinstance(sag_scale, (int, float)) or not math.isfinite(float(sag_scale)):
            raise ValueError(f"sag_scale={sag_scale!r}: a finite number (upstream's range is [0, 1]; sag_scale <= 0 is the plain pipeline)")
        return float(sag_scale)

    @classmethod
    def check_sag_args(cls, sag_scale=0.75, unet_config=None, weight_dtype="bf16"):
        """Everything ``enable_sag`` can refuse from the model alone, by name, without touching the GPU.  Returns the scale."""
        scale = cls.check_sag_scale(sag_scale)
        options.check(options.SAG, cls._model_options(unet_config, weight_dtype))
        return scale

    def enable_sag(self, sag_scale: float = 0.75):
        """Self-attention guidance (Hong et al. 2023; diffusers' ``StableDiffusionSAGPipeline``): every later step blurs the
        regions of the predicted x0 that the mid block's self-attention attends to (attention mass above its mean), re-noises
        them, runs the UNet once more on these degraded latents at the latent batch, and adds ``sag_scale * (m - d)`` to the
        guided prediction -- ``m`` the unconditional output under CFG, the conditional one without, ``d`` the output on the
        degraded latents.  Needs no negative prompt, so it also guides LCM-distilled UNets.  ``sag_scale`` given to a call
        overrides the default; ``sag_scale <= 0`` is the plain pipeline, bit for bit.  Valid with text-to-image,
        image-to-image, the 4-channel inpainting blend, all three prediction types, every scheduler, SD 2.x, FreeU, TAESD,
        HyperTile below the mid block, image sizes of 256 .. 1024 pixels per side in multiples of 64 and batch sharding;
        refused by name with PAG, ``guidance_rescale > 0``, Token Merging, T-GATE, DeepCache, IP-Adapter, ControlNet,
        HyperTile settings that tile the mid block, 9-channel inpainting UNets, fp8 and on the variant pipelines."""
        self._sag = self.check_sag_args(sag_scale, self.unet_config, self.weight_dtype)
        return self

    def disable_sag(self):
        """Later calls are those of a model that never saw SAG, bit for bit."""
        self._sag = None
        return self

    def _sag_check_call(self, sag_scale, guidance_rescale=0.0, control=None, ip_adapter_image=None, ip_adapter_image_embeds=None):
        """The SAG scale of one call -- the call's own value over ``enable_sag``'s, or None for a plain call (SAG off, or
        ``sag_scale <= 0``) -- and what a SAG call refuses, by name, before any GPU work."""
        if self._sag is None:
            if sag_scale is not None:
                raise ValueError("sag_scale given, but SAG is off: enable_sag() first")
            return None
        scale = self.check_sag_scale(self._sag if sag_scale is None else sag_scale)
        if scale <= 0.0:
            return None
        self.check_sag_args(scale, self.unet_config, self.weight_dtype)
        options.check(options.SAG, self._call_options(control, ip_adapter_image, ip_adapter_image_embeds, guidance_rescale))
        if self._hypertile is not None and self._hypertile[1] >= len(self.unet_config.block_out_channels) - 1:
            raise NotImplementedError(f"SAG with HyperTile max_depth={self._hypertile[1]} is refused: it tiles the mid block, whose "
                                      "whole-grid attention mass SAG reads")
        return scale

    def _sag_begin(self, batch_size, ctx):
        """Start of a sampling loop, before the context: capture onto the UNet handle with a mass buffer for the call's UNet
        batch, or off it.  A handle that never had it is not touched while SAG is off."""
        if self._sag_call is None:
            if getattr(self.unet, "_sag", False) or getattr(self.unet, "_sag_mass", None) is not None:
                self.unet.clear_sag()
            return
        mh, mw = self.unet.sag_mid_grid(self.unet_config, *self.latent_size)
        mass = torch.zeros((ctx.shape[0], mh * mw), dtype=torch.float32, device=self.unet.device)
        self.unet.set_sag(True, mass)

    def _sag_context(self, batch_size, ctx):
        """After the context of the first forward: the context of the SAG forward, the first ``batch_size`` prompt rows (the
        unconditional ones under CFG, else the conditional ones), in its own workspace -- once per call."""
        if self._sag_call is not None:
            self.unet.set_sag_context(ctx[:batch_size], *self.latent_size)

    # -- FreeU (diffusers enable_freeu) -----------------------------------------------------------------
    @staticmethod
    def check_freeu_args(s1, s2, b1, b2, weight_dtype="bf16"):
        """The arguments of ``enable_freeu`` checked, by name, without touching the GPU: four finite numbers > 0 (diffusers
        switches FreeU off silently when a factor is 0; here a factor <= 0 raises), and no fp8 UNet.  Returns
        ``(s1, s2, b1, b2)`` as floats."""
        return HipUNet2DConditionModel.check_freeu_args(s1, s2, b1, b2, weight_dtype)

    def enable_freeu(self, s1: float, s2: float, b1: float, b2: float):
        """FreeU (Si et al.; diffusers ``enable_freeu``): in every later call the resnets of up blocks 0 and 1 read the
        backbone features with their first half of the channels times ``b1`` / ``b2`` and the skip features with their four
        lowest Fourier modes times ``s1`` / ``s2`` (SD 1.x preset: 0.9, 0.2, 1.5, 1.6).  Valid with every pipeline, DeepCache,
        IP-Adapter, ControlNet, Token Merging, TAESD, every image size and batch sharding; refused on fp8 UNets."""
        self._freeu = self.check_freeu_args(s1, s2, b1, b2, self.weight_dtype)
        return self

    def disable_freeu(self):
        """Later calls are those of a model that never saw FreeU, bit for bit."""
        self._freeu = None
        return self

    def _freeu_begin(self):
        """Start of a sampling loop: the setting onto the UNet handle."""
        if self._freeu is None:
            self.unet.disable_freeu()
        else:
            self.unet.set_freeu(*self._freeu)

    # -- T-GATE (Zhang et al. 2024) --------------------------------------------------------
    @staticmethod
    def check_tgate_step(gate_step):
        """``gate_step`` of ``enable_tgate``: an integer >= 1 (``ValueError`` otherwise)."""
        if isinstance(gate_step, bool) or not isinstance(gate_step, int) or gate_step < 1:
            raise ValueError(f"gate_step={gate_step!r}: T-GATE takes an integer gate step >= 1 (steps 0 .. gate_step - 1 run with "
                             "cross-attention; a gate at or past the last step is the plain pipeline)")
        return gate_step

    @classmethod
    def check_tgate_args(cls, gate_step, unet_config=None, weight_dtype="bf16"):
        """Everything ``enable_tgate`` can refuse from the model alone, by name, without touching the GPU."""
        gate_step = cls.check_tgate_step(gate_step)
        options.check(options.TGATE, cls._model_options(unet_config, weight_dtype))
        return gate_step

    def enable_tgate(self, gate_step: int = 10):
        """T-GATE: every later call computes the prompt cross-attention in its first ``gate_step`` executed steps only.  The
        last of them also stores, per transformer block, the mean of the CFG pair's two cross-attention outputs; from step
        ``gate_step`` on the UNet runs on the latents alone -- half the batch under CFG, the stored tensor in place of
        norm2 and attn2, no classifier-free guidance and no ``guidance_rescale`` in the step.  ``gate_step`` at or past the
        number of steps that run is the plain pipeline.  Valid with text-to-image, image-to-image (the steps that run count)
        and 4-channel inpainting, every scheduler, LCM-distilled UNets, SD 2.x, Token Merging, FreeU and TAESD; refused by
        name with DeepCache, ControlNet, IP-Adapter, fp8 and 9-channel inpainting UNets and on the variant pipelines."""
        self._tgate_step = self.check_tgate_args(gate_step, self.unet_config, self.weight_dtype)
        return self

    def disable_tgate(self):
        """Later calls are those of a model that never saw T-GATE, bit for bit."""
        self._tgate_step = None
        return self

    def _tgate_check_call(self, control=None, ip_adapter_image=None, ip_adapter_image_embeds=None):
        """What a call with T-GATE on refuses, by name, before any GPU work."""
        if self._tgate_step is None:
            return
        self.check_tgate_args(self._tgate_step, self.unet_config, self.weight_dtype)
        options.check(options.TGATE, self._call_options(control, ip_adapter_image, ip_adapter_image_embeds))

    def _tgate_begin(self, latent_batch):
        """Start of a sampling loop: the UNet's workspace covers the capture plans while T-GATE is on.  A model that never
        enabled it asks nothing of the handle."""
        if self._tgate_step is not None:
            self.unet.reserve_tgate(latent_batch, *self.latent_size)
            self._tgate_reserved = True
        elif self._tgate_reserved:
            self.unet.reserve_tgate(None)
            self._tgate_reserved = False

    # -- loading ---------------------------------------------------------------------------
    @classmethod
    def from_pretrained(cls, pretrained_model_name_or_path, timestamps=None, safety_checker=None,
                        requires_safety_checker=False, torch_dtype=None, **kwargs):
        """``from_pretrained`` of the harness (``src/experiments/base_experiment.py:57-63``).

        A local diffusers directory is loaded; a model NAME is a network fetch and cannot be
        resolved offline, in which case SD-1.5-shaped synthetic weights seeded
        by ``SD_AMD_WEIGHTS_SEED`` (default 1234) are used and ``weights_source`` says so."""
        path = os.environ.get("SD_AMD_MODEL_DIR") or str(pretrained_model_name_or_path)
        # time_cond_proj_dim (YAML model.time_cond_proj_dim): shapes the synthetic stand-in of a hub name; a local checkpoint's
        # unet/config.json decides, and a different value is an error
        tcond = kwargs.pop("time_cond_proj_dim", None)
        # unet_arch (YAML model.unet_arch: "sd15" | "sd2"), with sample_size and prediction_type (YAML model.sample_size /
        # model.prediction_type): shape the stand-in of a hub name the same way -- "sd2" is the Stable Diffusion 2.x UNet
        # (weights.sd2_unet_config); a local checkpoint's own files decide, and a conflicting key is an error
        arch = kwargs.pop("unet_arch", None)
        ssize = kwargs.pop("sample_size", None)
        ptype = kwargs.pop("prediction_type", None)
        if arch not in (None, "sd15", "sd2"):
            raise ValueError(f"unet_arch={arch!r}: 'sd15' or 'sd2'")
        if os.path.isdir(path):
            has_clip = all(os.path.exists(os.path.join(path, *p)) for p in (("tokenizer", "vocab.json"),
                                                                            ("tokenizer", "merges.txt"),
                                                                            ("text_encoder", "model.safetensors")))
            kwargs.setdefault("scheduler", PNDMConfigStub(load_scheduler_config(path)))   # the checkpoint's own scheduler config
            ucfg = load_unet_config(path)
            have = ucfg.time_cond_proj_dim if ucfg is not None else None
            if tcond is not None and tcond != have:
                raise ValueError(f"time_cond_proj_dim={tcond} conflicts with the checkpoint {path!r} (its UNet has {have})")
            eff = ucfg or UNetConfig()
            is_sd2 = eff.heads_per_level == SD2_HEADS and eff.cross_attention_dim == SD2_CONTEXT_DIM
            if arch is not None and (arch == "sd2") != is_sd2:
                raise ValueError(f"unet_arch={arch!r} conflicts with the checkpoint {path!r} (heads {eff.heads_per_level}, "
                                 f"cross_attention_dim {eff.cross_attention_dim})")
            if ssize is not None and int(ssize) != eff.sample_size:
                raise ValueError(f"sample_size={ssize} conflicts with the checkpoint {path!r} (its UNet has {eff.sample_size})")
            sched_cfg = getattr(kwargs["scheduler"], "config", None)          # (a caller's scheduler: dict- or attribute-style config)
            have_p = (sched_cfg.get("prediction_type", "epsilon") if hasattr(sched_cfg, "get")
                      else getattr(sched_cfg, "prediction_type", "epsilon"))
            if ptype is not None and ptype != have_p:
                raise ValueError(f"prediction_type={ptype!r} conflicts with the checkpoint {path!r} (its scheduler has {have_p!r})")
            sd = load_unet_state_dict(path)
            check_projection_layout(eff, sd)
            return cls(unet_config=ucfg, state_dict=sd, source=f"local:{path}", clip_dir=path if has_clip else None, **kwargs)
        seed = int(os.environ.get("SD_AMD_WEIGHTS_SEED", "1234"))
        if arch == "sd2":
            if tcond is not None:
                raise ValueError("unet_arch='sd2' with time_cond_proj_dim: no LCM-distilled Stable Diffusion 2.x stand-in is built")
            kwargs.setdefault("unet_config", sd2_unet_config(sample_size=96 if ssize is None else int(ssize)))
        elif ssize is not None:
            kwargs.setdefault("unet_config", UNetConfig(sample_size=int(ssize), time_cond_proj_dim=tcond))
            tcond = None
        if ptype is not None:
            from .schedulers import SD15_SCHEDULER_CONFIG
            kwargs.setdefault("scheduler", PNDMConfigStub({**SD15_SCHEDULER_CONFIG, "prediction_type": str(ptype)}))
        if tcond is not None:
            kwargs.setdefault("unet_config", UNetConfig(time_cond_proj_dim=int(tcond)))
        return cls(weights_seed=seed, source=f"synthetic(seed={seed}) for {pretrained_model_name_or_path}", **kwargs)

    def _ensure_unet(self):
        if self.unet is None:
            sd = self._state_dict or make_synthetic_state_dict(self.unet_config, self._weights_seed)
            if self._ip_sd is not None:
                sd = {**sd, **self._ip_sd}
            for item in self._lora:
                if item[0] == "file":
                    from .weights import fuse_lora_state_dict
                    fuse_lora_state_dict(sd, item[1], item[2])
                    self.weights_source += " + LoRA(local file) fused"
                else:
                    _fuse_synthetic_lora(sd, *item)
                    self.weights_source += f" + SYNTHETIC low-rank stand-in for a hub LoRA (seed={item[0]}) fused"
            self.unet = HipUNet2DConditionModel(self.unet_config, sd, device="cuda:%d" % torch.cuda.current_device(),
                                                weight_dtype=self.weight_dtype)
            if self.unet.weight_dtype != "bf16":
                self.weights_source += f" [{self.unet.weight_dtype} weights + activations in the conv / FF / QKV contractions]"
            self._state_dict = None
            self._ip_sd = None

    def _ensure_vae(self):
        """AutoencoderKL decoder on libsdhip; local weights if the model directory has
        them, SD-1.5-shaped synthetic weights otherwise."""
        if self.vae_decoder is None:
            self._ensure_unet()
            cfg = VaeConfig(sample_size=self.unet_config.sample_size)
            path = os.environ.get("SD_AMD_MODEL_DIR", "")
            try:
                sd = load_vae_state_dict(path) if path and os.path.isdir(path) else None
            except FileNotFoundError:
                sd = None
            sd = sd or make_synthetic_vae_state_dict(cfg)
            self.vae_decoder = HipVaeDecoder(cfg, sd, device=str(self.unet.device))
        return self.vae_decoder

    def _ensure_vae_encoder(self):
        """AutoencoderKL encoder on libsdhip (image-to-image); weights from where the decoder's come from."""
        if self.vae_encoder is None:
            self._ensure_unet()
            cfg = VaeConfig(sample_size=self.unet_config.sample_size)
            path = os.environ.get("SD_AMD_MODEL_DIR", "")
            try:
                sd = load_vae_state_dict(path) if path and os.path.isdir(path) else None
            except FileNotFoundError:
                sd = None
            sd = sd or make_synthetic_vae_state_dict(cfg)
            self.vae_encoder = HipVaeEncoder(cfg, sd, device=str(self.unet.device))
        return self.vae_encoder

    # -- AutoencoderTiny (diffusers AutoencoderTiny = TAESD, upstream-recall) --------------------------------
    TINY_VAE_USES = ("all", "previews")

    def load_tiny_vae(self, pretrained_model_name_or_path, use_for: str = "all"):
        """A tiny autoencoder beside the AutoencoderKL, before or after the model moves to the GPU.  ``use_for="all"``: the
        final latents and every stored x0 preview are decoded by it (from the UNet's latents as they are: its scaling factor
        is 1), and image-to-image / inpainting take their image latents from its encoder, which has no posterior -- nothing
        is drawn for it, so the forward noise is the generator's FIRST draw (as diffusers with ``.latents``) and
        ``sample_mode`` is ignored.  ``use_for="previews"``: only the x0 previews use it; the final image and all encoding
        stay on the AutoencoderKL.  A local directory (``config.json`` + ``diffusion_pytorch_model.safetensors``) is read for
        real and must be the one structure that is built (``vae.check_tiny_vae_config``); a hub NAME is a network fetch, for
        which a seeded stand-in is used (``weights_source`` says so)."""
        from .vae import load_tiny_vae_state_dict
        if use_for not in self.TINY_VAE_USES:
            raise ValueError(f"use_for={use_for!r}: one of {self.TINY_VAE_USES}")
        if self.tiny_vae_use is not None:
            raise NotImplementedError("load_tiny_vae: a tiny VAE is already loaded (unload_tiny_vae first)")
        path = str(pretrained_model_name_or_path)
        if os.path.isdir(path):
            self._tiny_sd = load_tiny_vae_state_dict(path)
            self._tiny_source = f" + AutoencoderTiny(local:{path}, {use_for})"
        elif not self._looks_like_hub_name(path):
            raise FileNotFoundError(f"load_tiny_vae: no AutoencoderTiny directory at {path!r}")
        else:
            self._tiny_seed = int.from_bytes(hashlib.sha256(path.encode()).digest()[:4], "little")
            self._tiny_source = f" + SYNTHETIC stand-in for the hub AutoencoderTiny {path} (seed={self._tiny_seed}, {use_for})"
        self.tiny_vae_use = use_for
        self.weights_source += self._tiny_source

    def unload_tiny_vae(self):
        """Every path is the AutoencoderKL's again, bit for bit; the handles and their memory are dropped."""
        if self._tiny_source:
            self.weights_source = self.weights_source.replace(self._tiny_source, "", 1)
        self._tiny_sd = self._tiny_seed = self._tiny_source = None
        self.tiny_vae_use = None
        self.tiny_vae_decoder = self.tiny_vae_encoder = None

    def _tiny_state_dict(self):
        from .vae import make_synthetic_tiny_vae_state_dict
        if self._tiny_sd is None:
            self._tiny_sd = make_synthetic_tiny_vae_state_dict(seed=self._tiny_seed)
        return self._tiny_sd

    def _ensure_tiny_vae(self):
        if self.tiny_vae_decoder is None:
            from .vae import HipTinyVaeDecoder
            self._ensure_unet()
            self.tiny_vae_decoder = HipTinyVaeDecoder(self._tiny_state_dict(), device=str(self.unet.device))
        return self.tiny_vae_decoder

    def _ensure_tiny_vae_encoder(self):
        if self.tiny_vae_encoder is None:
            from .vae import HipTinyVaeEncoder
            self._ensure_unet()
            self.tiny_vae_encoder = HipTinyVaeEncoder(self._tiny_state_dict(), device=str(self.unet.device))
        return self.tiny_vae_encoder

    def _image_latents(self, img, shape, sample_mode, generator):
        """The scaled latents of an image in [0, 1] on the device: the AutoencoderKL's posterior (one draw of ``shape`` for
        ``sample_mode="sample"``), or, with a tiny VAE loaded for "all", its encoder's output as it is (no draw)."""
        if self.tiny_vae_use == "all":
            return self._ensure_tiny_vae_encoder().encode(img)
        enc = self._ensure_vae_encoder()
        moments = enc.encode(img)
        post = sdist.randn(shape, generator) if sample_mode == "sample" else None
        return enc.sample(moments, post, mode=sample_mode, scale=self.vae_config.scaling_factor)

    def to(self, device):
        """``model.to(device)`` (``base_experiment.py:64``; ``ddim.py:31,33``).  The UNet weights
        live in HBM for the life of the object (1.7 GB of 288 GB); ``to("cpu")`` is a no-op."""
        device = torch.device(device)
        if device.type == "cuda":
            self._ensure_unet()
            self.device = self.unet.device
            if self._clip_dir is not None:
                from .clip import ClipPromptEncoder
                self.text_encoder = ClipPromptEncoder.from_pretrained(self._clip_dir, device=str(self.device))
                self._clip_dir = None
        return self

    # LCM-LoRA hooks used by src/experiments/consistency_model.py:20-21
    def load_lora_weights(self, adapter_id, scale: float = 1.0, rank: int = 64):
        """A local LoRA file / directory (``pytorch_lora_weights.safetensors``) is read and fused for real
        (``weights.fuse_lora_state_dict``); a hub NAME is a network fetch, for which a seeded synthetic
        low-rank update of the same structure stands in."""
        if self.unet is not None:
            raise RuntimeError("load_lora_weights must be called before the model is moved to the GPU")
        path = str(adapter_id)
        if os.path.isdir(path):
            path = os.path.join(path, "pytorch_lora_weights.safetensors")
        if os.path.isfile(path):
            from safetensors.torch import load_file
            self._pending_lora = ("file", load_file(path), scale)
            return
        seed = int.from_bytes(hashlib.sha256(str(adapter_id).encode()).digest()[:4], "little")
        self._pending_lora = (seed, scale, rank)

    def fuse_lora(self):
        if getattr(self, "_pending_lora", None) is not None:
            self._lora.append(self._pending_lora)
            self._pending_lora = None

    # -- IP-Adapter image prompts (diffusers IPAdapterMixin, upstream-recall; DESIGN.md "IP-Adapter") ----------------------
    IP_ADAPTER_EMBED_DIM = 1024         # image_embeds width of the published ip-adapter_sd15 (CLIP ViT-H/14 projection)

    def load_ip_adapter(self, pretrained_model_name_or_path_or_dict, subfolder=None, weight_name=None,
                        image_encoder_folder="image_encoder"):
        """``pipe.load_ip_adapter(...)`` for ONE plain adapter (``ip-adapter_sd15``: ImageProjection, 4 image tokens).  Like
        ``load_lora_weights`` it must run before the model moves to the GPU.  A local file, or a local directory with
        ``[subfolder/]weight_name`` (``.safetensors`` or ``.bin``, upstream layout), is read for real and its
        ``image_encoder_folder`` -- relative to the subfolder as upstream resolves it, or to the directory -- serves
        ``ip_adapter_image``; a hub NAME is a network fetch, for which seeded synthetic adapter weights of the
        published shape stand in (``weights_source`` says so; only ``ip_adapter_image_embeds`` works then)."""
        import dataclasses
        from .weights import load_ip_adapter_state_dict, make_synthetic_ip_adapter_state_dict
        if self.unet is not None:
            raise RuntimeError("load_ip_adapter must be called before the model is moved to the GPU")
        src = pretrained_model_name_or_path_or_dict
        if isinstance(src, (list, tuple)) or isinstance(weight_name, (list, tuple)) or isinstance(subfolder, (list, tuple)):
            raise NotImplementedError("load_ip_adapter: several IP-Adapters at once are not built (one adapter, one image per sample)")
        if self._ip_loaded:
            raise NotImplementedError("load_ip_adapter: an adapter is already loaded (several at once are not built; unload_ip_adapter first)")
        if isinstance(src, dict):
            raise NotImplementedError("load_ip_adapter: pass a local file or directory (a state dict goes through "
                                      "weights.map_ip_adapter_state_dict)")
        path = str(src)
        base = self.unet_config
        if os.path.isdir(path):
            root = os.path.join(path, subfolder) if subfolder else path
            if weight_name is None:
                raise ValueError("load_ip_adapter: weight_name is needed with a directory (e.g. 'ip-adapter_sd15.safetensors')")
            file = os.path.join(root, weight_name)
        else:
            root, file = os.path.dirname(path), path
        if os.path.isfile(file):
            sd, e = load_ip_adapter_state_dict(file, base)
            self._ip_source = f" + IP-Adapter(local:{file})"
            if image_encoder_folder is not None:
                for cand in (os.path.join(root, image_encoder_folder), os.path.join(os.path.dirname(root), image_encoder_folder),
                             os.path.join(path, image_encoder_folder) if os.path.isdir(path) else None):
                    if cand and os.path.isfile(os.path.join(cand, "config.json")):
                        self._ip_encoder_dir = cand
                        break
        elif os.path.isdir(path) or not self._looks_like_hub_name(path):
            raise FileNotFoundError(f"load_ip_adapter: no adapter file at {file!r}")
        else:
            seed = int.from_bytes(hashlib.sha256(f"{path}/{subfolder}/{weight_name}".encode()).digest()[:4], "little")
            e = self.IP_ADAPTER_EMBED_DIM
            sd = make_synthetic_ip_adapter_state_dict(dataclasses.replace(base, ip_adapter_embed_dim=e), seed)
            self._ip_source = f" + SYNTHETIC stand-in for the hub IP-Adapter {path} (seed={seed})"
        self.weights_source += self._ip_source
        self.unet_config = dataclasses.replace(base, ip_adapter_embed_dim=e)
        self._ip_sd, self._ip_loaded = sd, True

    @staticmethod
    def _looks_like_hub_name(path: str) -> bool:
        """``name`` or ``org/name`` of hub characters, nothing that only a file system path has: not absolute, no ``.`` / ``..``
        / ``~`` component, no weight-file extension, no second separator.  Anything else that does not exist is a mistyped
        local path and raises, so that random stand-in weights never replace a checkpoint the caller meant to load."""
        import re
        if os.path.isabs(path) or path.lower().endswith((".safetensors", ".bin", ".pt", ".pth", ".ckpt")):
            return False
        parts = path.split("/")
        return 1 <= len(parts) <= 2 and all(re.fullmatch(r"[A-Za-z0-9][A-Za-z0-9._\-]*", q) and q != ".." for q in parts)

    def set_ip_adapter_scale(self, scale):
        """One float for every block (diffusers' per-block dicts are not built); applies from the next call on."""
        if isinstance(scale, (dict, list, tuple)):
            raise NotImplementedError("set_ip_adapter_scale: one float (per-block scale dicts and per-adapter lists are not built)")
        if isinstance(scale, bool) or not isinstance(scale, (int, float)) or not math.isfinite(float(scale)):
            raise ValueError(f"set_ip_adapter_scale: scale={scale!r} must be a finite number")
        self._ip_scale = float(scale)

    def unload_ip_adapter(self):
        """Calls run without an image prompt again (``ip_adapter_image*`` arguments are refused).  Before the model has
        moved to the GPU the adapter's weights are dropped as well; afterwards they stay in the handle, unused."""
        import dataclasses
        self._ip_loaded = False
        self._ip_encoder_dir, self._ip_encoder, self._ip_pending = None, None, None
        src = self._ip_source
        if src and self.weights_source.endswith(src):
            self.weights_source = self.weights_source[:-len(src)]
        elif src:
            self.weights_source = self.weights_source.replace(src, "", 1)
        self._ip_source = None
        if self.unet is None:
            self._ip_sd = None
            self.unet_config = dataclasses.replace(self.unet_config, ip_adapter_embed_dim=None, ip_adapter_tokens=None)
        else:
            self.unet.clear_ip_adapter()

    IP_ARGS_RULE = "ip_adapter_image and ip_adapter_image_embeds are exclusive: pass one of them"

    def _ip_adapter_args(self, ip_adapter_image, ip_adapter_image_embeds, batch_size: int, do_cfg: bool):
        """Every check of the two image-prompt arguments, on the host, before any GPU work.  Returns None (no image prompt),
        ("embeds", positive [B, E], negative [B, E] or None) or ("image", uint8 [B,3,H,W])."""
        if ip_adapter_image is None and ip_adapter_image_embeds is None:
            return None
        if ip_adapter_image is not None and ip_adapter_image_embeds is not None:
            raise ValueError(self.IP_ARGS_RULE)
        if not self._ip_loaded or self.unet_config.ip_adapter_embed_dim is None:
            raise ValueError("ip_adapter_image / ip_adapter_image_embeds need a loaded IP-Adapter (load_ip_adapter before the model "
                             "moves to the GPU)")
        e = self.unet_config.ip_adapter_embed_dim
        if ip_adapter_image_embeds is not None:
            emb = ip_adapter_image_embeds
            if isinstance(emb, (list, tuple)):
                if len(emb) != 1:
                    raise NotImplementedError(f"ip_adapter_image_embeds: a list of {len(emb)} (several IP-Adapters at once are not built)")
                emb = emb[0]
            if not torch.is_tensor(emb) or not emb.is_floating_point():
                raise ValueError("ip_adapter_image_embeds must be a float tensor or a one-element list of one")
            if emb.dim() == 3:
                if emb.shape[1] != 1:
                    raise NotImplementedError(f"ip_adapter_image_embeds {tuple(emb.shape)}: several images per sample are not built")
                emb = emb[:, 0]
            if emb.dim() != 2 or emb.shape[1] != e:
                raise ValueError(f"ip_adapter_image_embeds must be [B, {e}] or [B, 1, {e}] (E = {e} of the loaded adapter), got "
                                 f"{tuple(ip_adapter_image_embeds[0].shape if isinstance(ip_adapter_image_embeds, (list, tuple)) else ip_adapter_image_embeds.shape)}")
            emb = emb.detach().to("cpu", torch.float32)
            n, neg = int(emb.shape[0]), None
            if do_cfg and n == 2 * batch_size and batch_size >= 1 and n != 1:
                neg, emb = emb[:batch_size], emb[batch_size:]         # negative first, like the prompt
            elif n == 1:
                emb = emb.expand(batch_size, e)
            elif n != batch_size:
                raise ValueError(f"ip_adapter_image_embeds batch {n} does not match the prompt batch {batch_size} "
                                 f"(B, 1, or 2 B = negative | positive under CFG)")
            return ("embeds", emb, neg)
        img = ip_adapter_image
        if isinstance(img, (list, tuple)) and len(img) > 0 and isinstance(img[0], (list, tuple)):
            raise NotImplementedError("ip_adapter_image: nested lists (several IP-Adapters or several images per sample) are not built")
        if hasattr(img, "convert"):
            img = [img]
        if _is_pil_list(img):
            img = torch.from_numpy(_pil_stack(img, "RGB", "uint8", "ip_adapter_image: the PIL images")).permute(0, 3, 1, 2)
        if not torch.is_tensor(img) or img.dim() != 4 or img.shape[1] != 3:
            raise ValueError("ip_adapter_image must be a list of PIL images of one size or a uint8 / float [B,3,H,W] tensor")
        if img.is_floating_point():
            img = (img.clamp(0, 1) * 255.0).round().to(torch.uint8)       # (what VaeImageProcessor's 'pil' output holds)
        elif img.dtype != torch.uint8:
            raise ValueError(f"ip_adapter_image: dtype {img.dtype} (uint8, or floats in [0, 1])")
        if img.shape[0] == 1 and batch_size > 1:
            img = img.expand(batch_size, -1, -1, -1)
        if img.shape[0] != batch_size:
            raise ValueError(f"ip_adapter_image batch {img.shape[0]} does not match the prompt batch {batch_size}")
        self._ip_image_encoder_config()          # (refuses a missing or unbuilt encoder by name, still on the host)
        return ("image", img.contiguous())

    def _ip_image_encoder_config(self):
        """(ClipVisionConfig, hidden_act) of the adapter's ``image_encoder`` directory, checked against what the HIP vision
        tower builds and against the adapter's embed dim."""
        import json
        from .clip_score import ClipVisionConfig, check_vision_config
        d = self._ip_encoder_dir
        if d is None:
            raise ValueError("ip_adapter_image needs the adapter's image encoder: no local image_encoder directory was found by "
                             "load_ip_adapter (pass ip_adapter_image_embeds instead)")
        with open(os.path.join(d, "config.json"), encoding="utf-8") as f:
            j = json.load(f)
        j = {**j.get("vision_config", {}), **{k: v for k, v in j.items() if k != "vision_config"}}
        cfg = ClipVisionConfig(hidden_size=int(j["hidden_size"]), num_hidden_layers=int(j["num_hidden_layers"]),
                               num_attention_heads=int(j["num_attention_heads"]), intermediate_size=int(j["intermediate_size"]),
                               image_size=int(j.get("image_size", 224)), patch_size=int(j.get("patch_size", 14)),
                               projection_dim=int(j.get("projection_dim", 512)), layer_norm_eps=float(j.get("layer_norm_eps", 1e-5)),
                               hidden_act=str(j.get("hidden_act", "quick_gelu")))
        try:
            check_vision_config(cfg, extended=True)        # (also ViT-H/14: head dim 80, exact gelu)
        except ValueError as err:
            raise NotImplementedError(f"ip_adapter_image: the image encoder at {d!r} is not built by the HIP vision tower ({err}); "
                                      "pass ip_adapter_image_embeds") from None
        if cfg.projection_dim != self.unet_config.ip_adapter_embed_dim:
            raise ValueError(f"ip_adapter_image: the image encoder projects to {cfg.projection_dim}, the adapter takes "
                             f"E = {self.unet_config.ip_adapter_embed_dim}")
        return cfg

    def encode_ip_adapter_image(self, images: torch.Tensor) -> torch.Tensor:
        """uint8 [B,3,H,W] -> ``image_embeds`` [B, E] through the adapter's CLIP vision tower on libsdhip."""
        if self._ip_encoder is None:
            from safetensors.torch import load_file
            from .clip_score import HipClipVisionModel
            cfg = self._ip_image_encoder_config()
            sd = {k: v.float() for k, v in load_file(os.path.join(self._ip_encoder_dir, "model.safetensors")).items()}
            self._ip_encoder = HipClipVisionModel(cfg, sd, device=str(self.unet.device))
        return self._ip_encoder.encode(images)

    @staticmethod
    def shard_ip_adapter_args(kwargs: dict, lo: int, hi: int, n: int) -> dict:
        """A sharded harness call: the rows [lo, hi) of ``ip_adapter_image`` / ``ip_adapter_image_embeds`` ride with this
        rank's prompts (``dist.shard_range``), as ``image=`` does.  A batch of 1 is broadcast and stays; embeds with 2 n rows
        (negative | positive) are sliced per half."""
        out = dict(kwargs)

        def cut(v):
            if isinstance(v, (list, tuple)) and len(v) == 1 and torch.is_tensor(v[0]):
                return [cut(v[0])]
            if torch.is_tensor(v):
                if v.shape[0] == 2 * n and n > 1:
                    return torch.cat([v[lo:hi], v[n + lo:n + hi]])
                return v[lo:hi] if v.shape[0] == n and n > 1 else v
            if isinstance(v, (list, tuple)) and len(v) == n and n > 1:
                return list(v[lo:hi])
            return v
        for k in ("ip_adapter_image", "ip_adapter_image_embeds"):
            if out.get(k) is not None:
                out[k] = cut(out[k])
        return out

    def _apply_ip_adapter(self, do_cfg: bool):
        """After ``set_context`` of a call: fold this call's image prompt into the UNet, or clear the last call's."""
        ip, self._ip_pending = self._ip_pending, None
        if ip is None:
            if self.unet.config.ip_adapter_embed_dim is not None:
                self.unet.clear_ip_adapter()
            return
        dev = self.unet.device
        if ip[0] == "image":
            pos, neg = self.encode_ip_adapter_image(ip[1].to(dev)), None
        else:
            pos, neg = ip[1].to(dev), None if ip[2] is None else ip[2].to(dev)
        if do_cfg:
            emb = torch.cat([torch.zeros_like(pos) if neg is None else neg, pos])      # negative first; diffusers: zeros_like
        else:
            emb = pos
        self.ip_adapter_image_embeds = emb
        self.unet.set_ip_adapter(emb.contiguous(), self._ip_scale, *self.latent_size)

    # -- ControlNet (diffusers StableDiffusionControlNetPipeline, upstream-recall) ---------------------------
    def load_controlnet(self, pretrained_model_name_or_path):
        """ONE ControlNet beside the UNet, before or after the model moves to the GPU.  A local directory in the upstream
        layout (``config.json`` and ``diffusion_pytorch_model.safetensors`` / ``.bin``) is read for real and must pair with the
        UNet (``weights.read_controlnet_config``); a hub NAME is a network fetch, for which a seeded ControlNet of
        the UNet's shape with NON-zero zero convs stands in (``weights_source`` says so)."""
        from .weights import controlnet_config_for, load_controlnet
        src = pretrained_model_name_or_path
        if isinstance(src, (list, tuple)):
            raise NotImplementedError("load_controlnet: a list of ControlNets (Multi-ControlNet) is not built")
        if self._cn_cfg is not None:
            raise NotImplementedError("load_controlnet: a ControlNet is already loaded (several at once are not built; "
                                      "unload_controlnet first)")
        path = str(src)
        if os.path.isdir(path):
            self._cn_cfg, self._cn_sd = load_controlnet(path, self.unet_config)
            self._cn_source = f" + ControlNet(local:{path})"
        elif not self._looks_like_hub_name(path):
            raise FileNotFoundError(f"load_controlnet: no ControlNet directory at {path!r}")
        else:
            self._cn_seed = int.from_bytes(hashlib.sha256(path.encode()).digest()[:4], "little")
            self._cn_cfg = controlnet_config_for(self.unet_config)
            self._cn_source = f" + SYNTHETIC stand-in for the hub ControlNet {path} (seed={self._cn_seed})"
        self.weights_source += self._cn_source

    def unload_controlnet(self):
        """Calls run without a ControlNet again (``control_image`` is refused); the handle and its memory are dropped."""
        src = self._cn_source
        if src:
            self.weights_source = self.weights_source.replace(src, "", 1)
        self._cn_cfg = self._cn_sd = self._cn_seed = self._cn_source = None
        self.controlnet = None
        self._cn_run = None
        if self.unet is not None:
            self.unet.clear_control_residuals()

    def _ensure_controlnet(self):
        if self.controlnet is None:
            from .controlnet import HipControlNetModel
            from .weights import make_synthetic_controlnet_state_dict
            sd = self._cn_sd if self._cn_sd is not None else make_synthetic_controlnet_state_dict(self._cn_cfg, self._cn_seed)
            self.controlnet = HipControlNetModel(self._cn_cfg, sd, device=str(self.unet.device))
            self._cn_sd = None
        return self.controlnet

    CONTROL_WINDOW_RULE = "0 <= control_guidance_start < control_guidance_end <= 1"

    def _control_args(self, control_image, controlnet_conditioning_scale, control_guidance_start, control_guidance_end,
                      guess_mode, mask_image, n_prompt: int):
        """Every check of the ControlNet arguments of a call, on the host, before any GPU work.  Returns None (no control
        image) or dict(image [Bc,3,H,W] fp32 in [0,1] on the host, pil, scale, start, end)."""
        if guess_mode:
            raise NotImplementedError("guess_mode is not built")
        if control_image is None:
            return None
        if self._cn_cfg is None:
            raise ValueError("control_image needs a loaded ControlNet (load_controlnet)")
        for name, v in (("controlnet_conditioning_scale", controlnet_conditioning_scale),
                        ("control_guidance_start", control_guidance_start), ("control_guidance_end", control_guidance_end)):
            if isinstance(v, (list, tuple)):
                raise NotImplementedError(f"{name}: a list (Multi-ControlNet) is not built; one number")
            if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(float(v)):
                raise ValueError(f"{name}={v!r} must be a finite number")
        if not 0.0 <= float(control_guidance_start) < float(control_guidance_end) <= 1.0:
            raise ValueError(f"control_guidance_start={control_guidance_start}, control_guidance_end={control_guidance_end}: "
                             f"{self.CONTROL_WINDOW_RULE}")
        if mask_image is not None:
            raise NotImplementedError("control_image with mask_image (a ControlNet with inpainting) is not built")
        options.check(options.CONTROL, self._model_options(self.unet_config, self.weight_dtype) + self._enabled({options.DEEPCACHE}))
        img, pil = control_image, False
        if hasattr(img, "convert"):
            img = [img]
        if isinstance(img, (list, tuple)):
            if len(img) == 0 or not all(hasattr(im, "convert") for im in img):
                raise NotImplementedError("control_image: a list of tensors or of lists (Multi-ControlNet) is not built; one "
                                          "[B,3,H,W] tensor or a list of PIL images of one size")
            img, pil = self._image_tensor(list(img)), True
        if not torch.is_tensor(img) or img.dim() != 4 or img.shape[1] != 3 or not img.is_floating_point():
            raise ValueError("control_image must be a float tensor [B,3,H,W] in [0,1] or a list of PIL images of one size")
        if n_prompt is not None and img.shape[0] not in (1, n_prompt):
            raise ValueError(f"control_image batch {img.shape[0]} does not match the prompt batch {n_prompt}")
        return dict(image=img.detach().to("cpu", torch.float32), pil=pil, scale=float(controlnet_conditioning_scale),
                    start=float(control_guidance_start), end=float(control_guidance_end))

    @staticmethod
    def resize_control_image(img: torch.Tensor, height: int, width: int, pil: bool = False) -> torch.Tensor:
        """The control image at the call's size, as VaeImageProcessor.preprocess(image, height, width) resizes it upstream
        (``do_normalize=False``): PIL images with Lanczos, tensors with ``F.interpolate``'s default (nearest).  Already at
        that size: as it is."""
        if tuple(img.shape[2:]) == (height, width):
            return img
        if pil:
            import numpy as np
            from PIL import Image
            out = []
            for im in img:
                a = (im.permute(1, 2, 0).clamp(0, 1) * 255.0).round().to(torch.uint8).numpy()
                r = Image.fromarray(a).resize((width, height), resample=Image.LANCZOS)
                out.append(torch.from_numpy(np.asarray(r, dtype=np.float32) / 255.0).permute(2, 0, 1))
            return torch.stack(out)
        return torch.nn.functional.interpolate(img, size=(height, width))

    @staticmethod
    def shard_control_args(kwargs: dict, lo: int, hi: int, n: int) -> dict:
        """A sharded harness call: the rows [lo, hi) of ``control_image`` ride with this rank's prompts, as
        ``shard_ip_adapter_args`` slices the image prompt.  A batch of 1 is broadcast and stays."""
        out = dict(kwargs)
        v = out.get("control_image")
        if torch.is_tensor(v) and v.shape[0] == n and n > 1:
            out["control_image"] = v[lo:hi]
        elif isinstance(v, (list, tuple)) and len(v) == n and n > 1:
            out["control_image"] = list(v[lo:hi])
        return out

    def _apply_controlnet(self, ctx, cn):
        """After ``set_context`` of a call: the ControlNet's prompt and conditioning embedding (once per call) from the checked
        arguments ``cn`` (``_control_args``), or the plain plans if the call has no control image."""
        self._cn_run = None
        self.unet.clear_control_residuals()
        if cn is None or cn["scale"] == 0.0:
            return                           # (scale 0: neither the ControlNet nor the variant runs; the plain call, bit for bit)
        net = self._ensure_controlnet()
        h, w = self.latent_size
        img = self.resize_control_image(cn["image"], self._size[0], self._size[1], cn["pil"])
        self.control_image = img
        net.set_context(ctx, h, w)
        net.set_cond(img)                    # [1 or B, 3, H, W]: read modulo its batch, so both CFG halves see it
        self._cn_run = dict(scale=cn["scale"], start=cn["start"], end=cn["end"], keep=None)

    def _control_step(self, i: int, n_steps: int, latents, unet_batch: int, t) -> None:
        """Before the UNet forward of step ``i`` of ``n_steps``: run the ControlNet and hand its residuals to the UNet at
        ``controlnet_conditioning_scale * keep_i``; a step whose scale is 0 runs the plain plan."""
        run = self._cn_run
        if run is None:
            return
        if run["keep"] is None or len(run["keep"]) != n_steps:
            from .weights import control_keep
            run["keep"] = control_keep(n_steps, run["start"], run["end"])
        s = run["scale"] * run["keep"][i]
        if s == 0.0:
            self.unet.clear_control_residuals()
            return
        buf = self.controlnet.forward_residuals(latents, unet_batch, float(t))
        self.unet.set_control_residuals(buf, s, unet_batch, *self.latent_size)

    def _control_end(self) -> None:
        if self._cn_run is not None:
            self.unet.clear_control_residuals()
            self._cn_run = None

    # -- properties the harness reads --------------------------------------------------------
    @property
    def num_timesteps(self):
        return self._num_timesteps

    @property
    def guidance_scale(self):
        return self._guidance_scale

    @property
    def do_classifier_free_guidance(self):
        return self._guidance_scale > 1 and self.unet_config.time_cond_proj_dim is None

    # -- helpers of the loop -----------------------------------------------------------------
    def encode_prompt(self, prompt, device, do_cfg, negative_prompt=None, prompt_embeds=None,
                      negative_prompt_embeds=None):
        if prompt_embeds is None:
            prompts = [prompt] if isinstance(prompt, str) else list(prompt)
            prompt_embeds = self.text_encoder(prompts)
        if do_cfg and negative_prompt_embeds is None:
            n = prompt_embeds.shape[0]
            neg = negative_prompt if negative_prompt is not None else [""] * n
            neg = [neg] * n if isinstance(neg, str) else list(neg)
            negative_prompt_embeds = self.text_encoder(neg)
        to = lambda t: None if t is None else t.to(device, torch.float32)
        return to(prompt_embeds), to(negative_prompt_embeds)

    def prepare_latents(self, batch_size, num_channels, height, width, device, generator, latents=None):
        shape = (batch_size, num_channels, height // self.vae_scale_factor, width // self.vae_scale_factor)
        if latents is None:
            latents = sdist.randn(shape, generator)      # (the global batch's draw, sliced, under a sharded harness call)
        elif tuple(latents.shape[-2:]) != shape[-2:]:
            raise ValueError(f"latents {tuple(latents.shape)} do not match height x width = {height}x{width} "
                             f"(latent {shape[2]}x{shape[3]})")
        latents = latents.to(device, torch.float32)
        return (latents * self.scheduler.init_noise_sigma).contiguous()

    def __call__(self, *args, return_execution_time=True, **kwargs):
        result, execution_time, x0_preds = self.call(*args, **kwargs)
        if return_execution_time:
            return result, execution_time, x0_preds
        return result, x0_preds

    def guidance_condition(self, guidance_scale: float) -> Optional[torch.Tensor]:
        """``timestep_cond`` of the reference (``src/models.py:195-202``): the guidance embedding of ``guidance_scale - 1``
        ([1, time_cond_proj_dim] fp32) when the UNet has ``time_cond_proj_dim``, else None."""
        d = self.unet_config.time_cond_proj_dim
        if d is None:
            return None
        return get_guidance_scale_embedding(float(guidance_scale) - 1.0, d)

    # -- pieces shared by the four pipelines ------------------------------------------------------
    SIZE_RULE = "height and width must each be a multiple of 64 in [256, 1024]"

    def check_size(self, height: Optional[int], width: Optional[int]):
        """(height, width) in pixels for a pipeline call.  ``None`` is ``sample_size * 8`` (the default size, always
        accepted); any other value must follow ``SIZE_RULE``.  Raises ``ValueError`` naming the rule."""
        default = self.unet_config.sample_size * self.vae_scale_factor
        out = []
        for name, v in (("height", height), ("width", width)):
            if v is None or (isinstance(v, int) and not isinstance(v, bool) and v == default):
                out.append(default)
                continue
            if not isinstance(v, int) or isinstance(v, bool) or v % 64 or not 256 <= v <= 1024:
                raise ValueError(f"{name}={v!r}: {self.SIZE_RULE}")
            out.append(v)
        return out[0], out[1]

    def _begin(self, prompt, height, width, guidance_scale, negative_prompt, num_images_per_prompt, prompt_embeds,
               negative_prompt_embeds, guidance_rescale=0.0, timesteps=None, sigmas=None, ip_adapter_image=None,
               ip_adapter_image_embeds=None):
        """Steps 0-3 of the reference's ``call`` (``src/models.py:110-160``): argument checks, batch size,
        prompt encoding, CFG concat; uploads the prompt K/V projections.  Returns (device, batch, do_cfg, ctx).
        ``guidance_rescale`` is not validated (as upstream): the step rescales when CFG runs and it is > 0."""
        if num_images_per_prompt != 1 or timesteps is not None or sigmas is not None:
            raise NotImplementedError("custom timesteps / num_images_per_prompt are outside the reference's use")
        height, width = self.check_size(height, width)          # before any GPU work
        batch_size = _prompt_batch(prompt, prompt_embeds)
        self._ip_pending = self._ip_adapter_args(ip_adapter_image, ip_adapter_image_embeds, batch_size,
                                                 guidance_scale > 1 and self.unet_config.time_cond_proj_dim is None)
        self._size = (height, width)
        self._ensure_unet()
        if not self._fp8_calibrated:
            self.calibrate_fp8()        # fp8 handles only; shared by the four pipelines (all enter through _begin)
        device = self.unet.device
        self._guidance_scale = guidance_scale
        self.unet.set_timestep_cond(self.guidance_condition(guidance_scale))      # (None clears it)
        do_cfg = self.do_classifier_free_guidance
        prompt_embeds, negative_prompt_embeds = self.encode_prompt(
            prompt, device, do_cfg, negative_prompt, prompt_embeds, negative_prompt_embeds)
        ctx = torch.cat([negative_prompt_embeds, prompt_embeds]) if do_cfg else prompt_embeds   # :154-155
        if self._pag_call is not None:          # PAG: the perturbed branch, last, sees the positive prompt
            ctx = torch.cat([ctx, prompt_embeds])
        return device, batch_size, do_cfg, ctx

    @property
    def latent_size(self):
        """(h, w) of the latent of the current call (``_begin`` fixed the pixel size)."""
        return self._size[0] // self.vae_scale_factor, self._size[1] // self.vae_scale_factor

    def _start_loop(self, batch_size, device, generator, latents, ctx, cache_branch_id, control=None):
        """Initial latents at the call's size, DeepCache branch and prompt context of the UNet."""
        latents = self.prepare_latents(batch_size, LATENT_CHANNELS, self._size[0], self._size[1], device, generator, latents)
        # The settings of this call onto the UNet handle, before the context (they are part of the UNet's plans, T-GATE's of the
        # workspace that holds it): first those the call does not use go off, then those it uses go on -- the handle refuses
        # pairs (options.py), also between a setting the last call left on it and one this call brings
        begins = ((self._hypertile, self._hypertile_begin), (self._tome, self._tome_begin), (self._freeu, self._freeu_begin),
                  (self._tgate_step, lambda: self._tgate_begin(batch_size)),
                  (None if cache_branch_id == -1 else cache_branch_id, lambda: self.unet.set_deepcache(cache_branch_id)),
                  (self._pag_call, self._pag_begin), (self._sag_call, lambda: self._sag_begin(batch_size, ctx)))
        for going_on in (False, True):
            for setting, begin in begins:
                if (setting is not None) == going_on:
                    begin()
        self.unet.set_context(ctx, *self.latent_size)
        self._sag_context(batch_size, ctx)
        self._apply_ip_adapter(ctx.shape[0] == 2 * batch_size and self.do_classifier_free_guidance)
        self._apply_controlnet(ctx, control)
        return latents

    def _eps_buffer(self, unet_batch, device):
        c = self.unet_config
        h, w = self.latent_size
        return torch.empty((unet_batch, c.out_channels, h, w), dtype=torch.float32, device=device)

    def _sample(self, steps, latents, unet_batch, do_cfg, guidance_scale, eta=0.0, generator=None, guidance_rescale=0.0,
                step_noise=None, collect_x0=True, deepcache=None, inpaint=None):
        """THE denoising loop (``src/models.py:210-282``) of all four pipelines, after ``_start_loop``.  ``steps``: the steps
        that run, each ``(t, scheduler, hand_off)`` -- ``hand_off`` is the scheduler whose multistep history receives the
        step's noise prediction (``_push_history``), or None.  ``deepcache``: the helper, whose plan indexes the timesteps
        that run (first match, as DeepCache's ``list.index``: both steps of PNDM's duplicated timestep get its first index).
        ``inpaint = (image latents, noise, latent mask)``: the step blends the kept region back in, noised to the next
        timestep that runs.  Returns (latents, x0 predictions of the first sample, seconds): the wall-clock of the loop only
        (``:208,284-285``), bracketed by device synchronisation."""
        device = self.unet.device
        sag = self._sag_call
        # SAG: the eps buffer holds the prediction on the degraded latents behind the first forward's rows
        eps = self._eps_buffer(unet_batch + (latents.shape[0] if sag is not None else 0), device)
        eps1 = eps[:unet_batch] if sag is not None else eps
        if sag is not None:
            mh, mw = self.unet.sag_mid_grid(self.unet_config, *self.latent_size)
            x_deg = torch.empty_like(latents, dtype=torch.float32)
            self.sag_masses = []
        ts = [s[0] for s in steps]
        n = len(steps)
        # T-GATE: steps 0 .. g - 1 as ever (step g - 1 also captures), steps g .. n - 1 gated: the UNet at the latent batch,
        # no CFG in the step, the model output in the first rows of the eps buffer.  g = None: off, or a gate the run never reaches.
        g = self._tgate_step if self._tgate_step is not None and self._tgate_step < n else None
        lb = latents.shape[0]
        x0_preds = []
        torch.cuda.synchronize(device)
        start_time = time.time()                                                                   # :208
        try:
            for i, (t, sched, hand_off) in enumerate(steps):                                       # :211
                ub, cfg, out = unet_batch, do_cfg, eps1
                if g is not None:
                    if i == g - 1:
                        self.unet.set_tgate(self.unet.TGATE_CAPTURE, lb, *self.latent_size)
                    elif i == g:
                        self.unet.set_tgate(self.unet.TGATE_REUSE, lb, *self.latent_size)
                    if i >= g:
                        ub, cfg, out = lb, False, eps[:lb]
                mode = CACHE_OFF
                if deepcache is not None:
                    mode = CACHE_FULL_AND_STORE if ts.index(t) % deepcache.cache_interval == 0 else CACHE_SKIP     # (A.5)
                self._control_step(i, n, latents, ub, t)
                self._tome_step()
                if sag is not None:
                    self.unet.set_sag(True)
                self.unet.forward_latents(latents, ub, float(t), out=out, cache_mode=mode)         # :217-235
                kw = {}
                if sag is not None:
                    # the first LB rows of the forward (uncond under CFG, else cond) and their masses -> degraded latents ->
                    # the UNet at the latent batch with those rows' prompt, capture off, into the last LB rows of eps
                    x32 = latents if latents.dtype == torch.float32 and latents.is_contiguous() else latents.float().contiguous()
                    sag_degrade(x32, eps[:lb], self.unet._sag_mass, mh, mw, sched.config.prediction_type,
                                float(sched.alphas_cumprod[int(t)]), out=x_deg)
                    if self._sag_keep:
                        self.sag_masses.append(self.unet._sag_mass[:lb].view(lb, mh, mw).clone())
                    self.unet.set_sag(False)
                    self.unet.forward_latents(x_deg, lb, float(t), out=eps[unet_batch:], sag_forward=True)
                    out = eps
                    kw["sag_scale"] = sag
                if step_noise is not None and i < n - 1 and "timestep_scaling" in getattr(sched, "config", ()):    # (LCM)
                    kw["noise"] = step_noise[i]             # indexed by EXECUTED step
                if cfg and guidance_rescale > 0.0:                                                 # :244-250
                    kw["guidance_rescale"] = guidance_rescale
                if inpaint is not None:
                    kw["inpaint"] = (*inpaint, ts[i + 1] if i + 1 < n else None)
                if self._pag_call is not None:              # (the eps buffer holds the perturbed third behind the CFG pair)
                    kw["pag_scale"] = pag_step_scale(*self._pag_call, t)
                step = sched.step_fused(out, guidance_scale, latents, t, cfg=cfg, eta=eta, generator=generator, **kw)   # :238-261
                latents = step[0]
                if collect_x0 and len(step) > 1:            # (PNDM returns no x0, :257-261)
                    x0_preds.append(step[1][0:1])
                if hand_off is not None:                    # :603-611, :1025-1033, :1045-1053
                    _push_history(hand_off, _combined(out, cfg, guidance_scale, sched), latents)
        finally:
            if g is not None:
                self.unet.set_tgate(self.unet.TGATE_OFF)
            if sag is not None:
                self.unet.set_sag(False)
            self._control_end()         # (also when a step raised: no residuals stay on the handle for the next call)
        torch.cuda.synchronize(device)
        return latents, x0_preds, time.time() - start_time                                        # :284-285

    def _run(self, a, ts_host, latents, unet_batch, do_cfg, inpaint=None):
        """The loop of this class's three kinds of call over ``ts_host`` with ``self.scheduler``, and the decode."""
        self._num_timesteps = len(ts_host)
        latents, x0_preds, execution_time = self._sample(
            [(t, self.scheduler, None) for t in ts_host], latents, unet_batch, do_cfg, a.guidance_scale, a.eta, a.generator,
            a.guidance_rescale, a.step_noise, a.collect_x0, self._deepcache, inpaint)
        return self._finish(latents, x0_preds, a.output_type, a.return_dict, execution_time)

    def _finish(self, latents, x0_preds, output_type, return_dict, execution_time):
        """``src/models.py:287-335``: decode (outside the timed loop), post-process, 3-tuple."""
        if output_type == "latent":
            image = latents
            image_x0 = x0_preds
        elif output_type in ("pt", "np", "pil"):
            def decoder(tiny: bool):
                """Latents -> the clamped [0, 1] picture.  A tiny VAE (load_tiny_vae) decodes the UNet's latents as they are."""
                if tiny:
                    vae = self._ensure_tiny_vae()
                    return lambda x: vae.decode(x, unit_range=True)
                vae, inv = self._ensure_vae(), 1.0 / self.vae_config.scaling_factor
                return lambda x: (vae.decode(x, inv) / 2 + 0.5).clamp(0, 1)                                  # :288,:312
            preview = decoder(True) if self.tiny_vae_use == "previews" else None
            decode = decoder(self.tiny_vae_use == "all")
            image = postprocess_images(decode(latents), output_type)
            # the reference decodes EVERY stored x0 prediction as well (:296-302)
            image_x0 = [postprocess_images((preview or decode)(x), output_type) for x in x0_preds]
        else:
            raise NotImplementedError(f"output_type {output_type!r}: 'latent', 'pt', 'np' and 'pil' are built")
        if not return_dict:
            return (image, None), execution_time, image_x0
        return StableDiffusionPipelineOutput(images=image, nsfw_content_detected=None), execution_time, image_x0

    # fixed calibration inputs: the SAME on every rank, for every prompt order, shard size and schedule
    FP8_CALIBRATION_SEED = 20240229
    FP8_CALIBRATION_PROMPTS = ("", "a photograph of an astronaut riding a horse")
    FP8_CALIBRATION_TIMESTEPS = (999.0, 499.0, 1.0)
    FP8_CALIBRATION_GUIDANCE = 8.0      # UNets with time_cond_proj_dim: the guidance scale the calibration forwards embed

    def calibrate_fp8(self, scales=None, margin: float = 2.0):
        """fp8 handles (``weight_dtype="fp8"``): fix the per-tensor e4m3 activation scales, ONCE and deterministically.
        ``scales`` given (e.g. saved from an earlier run: ``model.fp8_scales``): they are loaded through
        ``sd_unet_set_fp8_scale``.  Otherwise they come from the amax observed on a fixed calibration batch -- two latents
        drawn from a generator seeded with ``FP8_CALIBRATION_SEED``, the text encoder's embeddings of two fixed prompts, no
        CFG, the guidance embedding of ``FP8_CALIBRATION_GUIDANCE`` for a UNet with ``time_cond_proj_dim``, at three fixed
        timesteps (``sd_unet_calibrate_fp8``, margin 2) -- so every rank of a sharded run, whatever its
        shard, and every world size end up with the SAME scales (dist.py's invariant: an image does not depend on the
        world size; round 3 calibrated on the first call's own inputs, which differ per rank).  Runs outside any timed
        region; ``SD_AMD_FP8_CALIBRATE=0`` keeps the static defaults (clipping at |x| > 56 / 224)."""
        self._ensure_unet()
        if self.unet.weight_dtype != "fp8_e4m3":
            self._fp8_calibrated = True
            return {}
        if scales is not None:
            self.unet.set_fp8_scales(scales)
            how = "loaded"
        elif os.environ.get("SD_AMD_FP8_CALIBRATE", "1") == "0":
            self._fp8_calibrated = True
            return {}
        else:
            cfgu = self.unet_config
            g = torch.Generator().manual_seed(self.FP8_CALIBRATION_SEED)
            lat = torch.randn((2, LATENT_CHANNELS, cfgu.sample_size, cfgu.sample_size), generator=g)
            ctx = self.text_encoder(list(self.FP8_CALIBRATION_PROMPTS)).to(self.unet.device, torch.float32)
            branch = self.unet.cache_branch_id
            self.unet.set_deepcache(-1)             # the calibration pass runs the plan without DeepCache
            if cfgu.ip_adapter_embed_dim is not None:
                self.unet.clear_ip_adapter()        # ... and without an image prompt: the scales do not depend on the call's image
            self.unet.set_context(ctx)
            self.unet.set_timestep_cond(self.guidance_condition(self.FP8_CALIBRATION_GUIDANCE))
            if cfgu.in_channels == 9:
                # an inpainting UNet: a FIXED condition beside the fixed latents -- repaint everything (mask of ones) over a
                # blank masked image (zero latents) -- so the scales stay independent of rank and call
                s_ = cfgu.sample_size
                self.unet.set_inpaint_cond(torch.ones(2, 1, s_, s_), torch.zeros(2, LATENT_CHANNELS, s_, s_))
            self.unet.calibrate_fp8(lat, 2, list(self.FP8_CALIBRATION_TIMESTEPS), margin=margin)
            if cfgu.in_channels == 9:
                self.unet.clear_inpaint_cond()      # (the caller sets its own inpainting condition)
            self.unet.set_timestep_cond(None)
            self.unet.set_deepcache(branch)         # (the caller sets its own context and condition next)
            how = "calibrated on the fixed seeded batch"
        self.fp8_scales = dict(self.unet.fp8_scales())
        self._fp8_calibrated = True
        if "e4m3 activation scales" not in self.weights_source:
            self.weights_source += f" (per-tensor e4m3 activation scales {how})"
        return self.fp8_scales

    # -- image-to-image (diffusers StableDiffusionImg2ImgPipeline, upstream-recall) -----------------------------------
    @staticmethod
    def img2img_steps(num_inference_steps: int, strength: float):
        """``get_timesteps`` of diffusers' StableDiffusionImg2ImgPipeline: ``init = min(int(N * strength), N)``,
        ``t_start = max(N - init, 0)``; returns ``(t_start, steps that run = N - t_start)``.  ``strength`` outside [0, 1]
        and a combination that leaves no step to run raise ``ValueError``."""
        if isinstance(strength, bool) or not isinstance(strength, (int, float)) or not 0.0 <= float(strength) <= 1.0:
            raise ValueError(f"strength={strength!r}: the value of strength should be in [0.0, 1.0]")
        n = int(num_inference_steps)
        init = min(int(n * float(strength)), n)
        t_start = max(n - init, 0)
        if n - t_start < 1:
            raise ValueError(f"strength={strength} with num_inference_steps={n} leaves {n - t_start} steps to run; "
                             "image-to-image needs at least one (int(num_inference_steps * strength) >= 1)")
        return t_start, n - t_start

    @staticmethod
    def _image_tensor(image) -> torch.Tensor:
        """``image`` of a pipeline call -> fp32 [B, 3, H, W] in [0, 1] on the host: a float tensor as it is, a list of PIL
        images of one size through ``/ 255`` (VaeImageProcessor.pil_to_numpy)."""
        if isinstance(image, torch.Tensor):
            if image.dim() != 4 or image.shape[1] != 3 or not image.is_floating_point():
                raise ValueError(f"image must be a float tensor [B,3,H,W] in [0,1], got {tuple(image.shape)} {image.dtype}")
            return image
        if _is_pil_list(image):
            arr = _pil_stack(image, "RGB", "float32", "image: the PIL images") / 255.0
            return torch.from_numpy(arr).permute(0, 3, 1, 2).contiguous()
        raise ValueError("image must be a float tensor [B,3,H,W] in [0,1] or a list of PIL images of one size")

    def _img2img_args(self, prompt, image, strength, a, latents):
        """Every argument check of an image-to-image call (``a``: the arguments of ``call``), before any GPU work.  Returns
        (image tensor on the host, height, width, t_start)."""
        from .schedulers import PNDMScheduler
        if latents is not None:
            raise ValueError("image and latents are exclusive: the start latents of an image-to-image call are the noised "
                             "encoding of the image")
        if isinstance(self.scheduler, PNDMScheduler) or not hasattr(self.scheduler, "add_noise"):
            raise NotImplementedError(f"image= with {type(self.scheduler).__name__} is not built: PNDMScheduler duplicates its "
                                      "second timestep, and a schedule sliced at t_start changes what its PLMS warm-up means "
                                      "(DDIM, DPM-Solver and LCM are built)")
        if a.sample_mode not in ("sample", "argmax"):
            raise ValueError(f"sample_mode={a.sample_mode!r}: 'sample' or 'argmax'")
        t_start, _ = self.img2img_steps(a.num_inference_steps, strength)
        img = self._image_tensor(image)
        ih, iw = int(img.shape[2]), int(img.shape[3])
        self.check_size(ih, iw)                  # the image's sides obey SIZE_RULE like height / width
        for name, v, iv in (("height", a.height, ih), ("width", a.width, iw)):
            if v is not None and v != iv:
                raise ValueError(f"{name}={v} disagrees with the image ({ih}x{iw}): the image defines the size of the call")
        n_prompt = _prompt_batch(prompt, a.prompt_embeds)
        if img.shape[0] != n_prompt:
            raise ValueError(f"image batch {img.shape[0]} does not match the prompt batch {n_prompt}")
        return img, ih, iw, t_start

    def _img2img_start(self, img, sample_mode, generator, device, first_timestep):
        """Steps of StableDiffusionImg2ImgPipeline.prepare_latents, in upstream's order: encode, draw the posterior noise,
        draw the forward noise, ``add_noise`` at the first timestep that runs.  Both draws go through ``dist.randn`` (the
        global batch's draws under a sharded harness call).  Returns (noised start latents, clean scaled latents)."""
        shape = (img.shape[0], LATENT_CHANNELS, img.shape[2] // self.vae_scale_factor, img.shape[3] // self.vae_scale_factor)
        init = self._image_latents(img.to(device), shape, sample_mode, generator)
        noise = sdist.randn(shape, generator)
        return self.scheduler.add_noise(init, noise, first_timestep), init

    def _begin_call(self, prompt, height, width, a):
        """``_begin`` with the arguments ``a`` of ``call``, then the schedule.  Returns (device, batch, do_cfg, ctx)."""
        begun = self._begin(prompt, height, width, a.guidance_scale, a.negative_prompt, a.num_images_per_prompt, a.prompt_embeds,
                            a.negative_prompt_embeds, a.guidance_rescale, a.timesteps, a.sigmas, a.ip_adapter_image,
                            a.ip_adapter_image_embeds)
        self.scheduler.set_timesteps(a.num_inference_steps, device=begun[0])                    # :167-169
        return begun

    def _cache_branch(self) -> int:
        dc = self._deepcache
        return dc.cache_branch_id if dc is not None else -1

    @torch.no_grad()
    def _call_img2img(self, prompt, image, strength, a):
        """The loop of ``call`` (``a``: its arguments) started part-way down the schedule from a noised encoding of ``image``
        (SDEdit).  The schedule is the full ``num_inference_steps`` one; the last ``N - t_start`` of its timesteps run.  A
        multistep scheduler starts with a fresh history at that index (``_index_of`` resolves it from the timestep) while its
        lower-order rules at the end still count against the full schedule.  DeepCache's plan indexes the list that runs,
        so the first executed step is a full one."""
        img, ih, iw, t_start = self._img2img_args(prompt, image, strength, a, a.latents)
        device, batch_size, do_cfg, ctx = self._begin_call(prompt, ih, iw, a)
        ts_host = list(self.scheduler._timesteps_list)[t_start * self.scheduler.order:]
        # encoding and noising sit outside the timed region, as text encoding does
        start, _ = self._img2img_start(img, a.sample_mode, a.generator, device, ts_host[0])
        self.img2img_start_latents = start
        latents = self._start_loop(batch_size, device, None, start, ctx, self._cache_branch(), a.control)
        return self._run(a, ts_host, latents, ctx.shape[0], do_cfg)
    # -- inpainting (diffusers StableDiffusionInpaintPipeline, upstream-recall; DESIGN.md "Inpainting") ------------------
    @staticmethod
    def _mask_tensor(mask_image) -> torch.Tensor:
        """``mask_image`` of a pipeline call -> fp32 [B, 1, H, W] in [0, 1] on the host: a float tensor [B,1,H,W] or
        [B,H,W] as it is, a list of PIL images of one size through ``convert("L")`` and ``/ 255``."""
        if isinstance(mask_image, torch.Tensor):
            m = mask_image
            if m.dim() == 3:
                m = m[:, None]
            if m.dim() != 4 or m.shape[1] != 1 or not m.is_floating_point():
                raise ValueError(f"mask_image must be a float tensor [B,1,H,W] or [B,H,W] in [0,1], got "
                                 f"{tuple(mask_image.shape)} {mask_image.dtype}")
            return m.to(torch.float32)
        if _is_pil_list(mask_image):
            arr = _pil_stack(mask_image, "L", "float32", "mask_image: the PIL masks") / 255.0
            return torch.from_numpy(arr)[:, None].contiguous()
        raise ValueError("mask_image must be a float tensor [B,1,H,W] or [B,H,W] in [0,1] or a list of PIL images of one size")

    def _inpaint_args(self, prompt, image, mask_image, strength, a):
        """Every argument check of an inpainting call, before any GPU work: those of image-to-image, then the mask's.
        Returns (image, mask [B,1,H,W], height, width, t_start), tensors on the host."""
        img, ih, iw, t_start = self._img2img_args(prompt, image, strength, a, None)
        mask, latents = self._mask_tensor(mask_image), a.latents
        if tuple(mask.shape[2:]) != (ih, iw):
            raise ValueError(f"mask_image size {int(mask.shape[2])}x{int(mask.shape[3])} does not match the image size {ih}x{iw}")
        if mask.shape[0] != img.shape[0]:
            raise ValueError(f"mask_image batch {mask.shape[0]} does not match the image batch {img.shape[0]}")
        if latents is not None:
            if float(strength) != 1.0:
                raise ValueError(f"latents= with mask_image is the forward noise of the call and is accepted only at strength == "
                                 f"1.0 (got strength={strength}): below it the loop would start from pure noise part-way down "
                                 "the schedule")
            want = (img.shape[0], LATENT_CHANNELS, ih // self.vae_scale_factor, iw // self.vae_scale_factor)
            if tuple(latents.shape) != want:
                raise ValueError(f"latents {tuple(latents.shape)} do not match the image: expected {want}")
        return img, mask, ih, iw, t_start

    def inpaint_prepare(self, image: torch.Tensor, mask: torch.Tensor):
        """``sd_inpaint_prepare`` (one launch): (masked image [B,3,H,W] in the encoder's [0, 1] domain -- 0.5 where the
        mask is >= 0.5 --, latent mask [B,1,H/8,W/8] fp32 0 / 1 = the binarised mask's pixel (8i, 8j))."""
        from . import _lib
        lib = _lib.load()
        self._ensure_unet()
        img = image.to(self.unet.device, torch.float32).contiguous()
        m = mask.to(self.unet.device, torch.float32).contiguous()
        b, _, h, w = img.shape
        if h % 8 or w % 8 or tuple(m.shape) != (b, 1, h, w):
            raise ValueError(f"inpaint_prepare: image {tuple(img.shape)} (sides multiples of 8) and mask {tuple(m.shape)}")
        masked = torch.empty_like(img)
        lmask = torch.empty((b, 1, h // 8, w // 8), dtype=torch.float32, device=img.device)
        _lib.check(lib.sd_inpaint_prepare(_lib.current_stream(), img.data_ptr(), m.data_ptr(), masked.data_ptr(),
                                          lmask.data_ptr(), b, h, w), "sd_inpaint_prepare")
        return masked, lmask

    @torch.no_grad()
    def _call_inpaint(self, prompt, image, mask_image, strength, a):
        """The loop of ``_call_img2img`` with a mask (1 = repaint, 0 = keep).  A 4-channel UNet: after every step the kept
        region is replaced by the image's latents noised to the NEXT timestep (the image's latents themselves after the last
        step) -- inside the step's launch (the ``inpaint`` blend of ``_sample``).  A 9-channel UNet reads the latent mask and
        the masked image's latents as input channels 4..8 (``set_inpaint_cond``, once per call) and the loop does not blend.
        Draws, in order: posterior noise of the image latents, forward noise (or ``latents``), and for a 9-channel UNet the
        posterior noise of the masked-image latents."""
        img, mask, ih, iw, t_start = self._inpaint_args(prompt, image, mask_image, strength, a)
        device, batch_size, do_cfg, ctx = self._begin_call(prompt, ih, iw, a)
        nine = self.unet_config.in_channels == 9
        ts_host = list(self.scheduler._timesteps_list)[t_start * self.scheduler.order:]
        # mask processing, encoding and noising sit outside the timed region, as text encoding does
        img = img.to(device)
        masked_img, lmask = self.inpaint_prepare(img, mask)
        shape = (batch_size, LATENT_CHANNELS, ih // self.vae_scale_factor, iw // self.vae_scale_factor)
        init = None
        if not (nine and a.latents is not None):        # (9 channels from given noise at strength 1: nothing reads them)
            init = self._image_latents(img, shape, a.sample_mode, a.generator)
        noise = (a.latents if a.latents is not None else sdist.randn(shape, a.generator)).to(device, torch.float32).contiguous()
        if nine:
            masked_latents = self._image_latents(masked_img, shape, a.sample_mode, a.generator)
            self.unet.set_inpaint_cond(lmask, masked_latents)
        # upstream: pure noise (times init_noise_sigma, in _start_loop) at strength 1, the noised image latents below it
        start = noise if float(strength) == 1.0 else self.scheduler.add_noise(init, noise, ts_host[0])
        self.inpaint_image_latents, self.inpaint_latent_mask = init, lmask
        latents = self._start_loop(batch_size, device, None, start, ctx, self._cache_branch())
        self.img2img_start_latents = latents
        return self._run(a, ts_host, latents, ctx.shape[0], do_cfg, None if nine else (init, noise, lmask))

    # -- the sampling loop (src/models.py:32-335) ----------------------------------------------
    @torch.no_grad()
    def call(self, prompt: Union[str, List[str]] = None, height: Optional[int] = None, width: Optional[int] = None,
             num_inference_steps: int = 50, timesteps=None, sigmas=None, guidance_scale: float = 7.5,
             negative_prompt=None, num_images_per_prompt: int = 1, eta: float = 0.0, generator=None,
             latents: Optional[torch.Tensor] = None, prompt_embeds: Optional[torch.Tensor] = None,
             negative_prompt_embeds: Optional[torch.Tensor] = None, output_type: str = "pil",
             return_dict: bool = True, guidance_rescale: float = 0.0, step_noise: Optional[torch.Tensor] = None,
             collect_x0: bool = True, image=None, strength=STRENGTH_UNSET, sample_mode: str = "sample", mask_image=None,
             padding_mask_crop=None, ip_adapter_image=None, ip_adapter_image_embeds=None, control_image=None,
             controlnet_conditioning_scale=1.0, control_guidance_start=0.0, control_guidance_end=1.0, guess_mode=False,
             pag_scale=None, pag_adaptive_scale=None, sag_scale=None, **kwargs):
        """``control_image`` ([B,3,H,W] floats in [0,1], rgb, or a list of PIL images of one size; resized to the call's size
        as upstream resizes it, replicated over the batch, seen by both CFG halves): the structure condition of a loaded
        ControlNet (``load_controlnet``) for text-to-image and image-to-image.  Step i of N runs the ControlNet at
        ``controlnet_conditioning_scale * keep_i``, ``keep_i = 1 - float(i / N < control_guidance_start or (i + 1) / N >
        control_guidance_end)``; a step whose scale is 0 runs the plain UNet plan, bit for bit.

        ``ip_adapter_image`` (PIL images or uint8 / float [B,3,H,W]) or ``ip_adapter_image_embeds`` ([B, E], [B, 1, E] or
        [2 B, ...] negative first under CFG; a tensor or a one-element list): the image prompt of a loaded IP-Adapter
        (``load_ip_adapter``), for every kind of call below.

        ``image`` ([B,3,H,W] floats in [0,1], or a list of PIL images of one size): image-to-image with the semantics
        of diffusers' StableDiffusionImg2ImgPipeline -- the image defines the size, ``strength`` in [0, 1] how far up the
        schedule its encoding is noised (``img2img_steps``), ``sample_mode`` whether the posterior is sampled or its mode
        taken (ignored with a tiny VAE loaded for "all": its encoder has no posterior, see ``load_tiny_vae``).
        ``mask_image`` ([B,1,H,W] or [B,H,W] floats in [0,1], or PIL images; 1 = repaint, 0 = keep) beside ``image``:
        inpainting with the semantics of StableDiffusionInpaintPipeline (``_call_inpaint``); ``strength`` then defaults to 1.0
        instead of 0.8, and ``latents`` is the forward noise (strength 1.0 only).  A UNet with 9 input channels runs only with
        ``mask_image``.  ``image is None``: text-to-image, the path below."""
        if padding_mask_crop is not None:
            raise NotImplementedError("padding_mask_crop is not built (the crop-and-paste of StableDiffusionInpaintPipeline; "
                                      "without it upstream composites nothing in pixel space, and neither does this)")
        # (neither a prompt nor embeds: _begin refuses the call by name)
        n_prompt = None if prompt is None and prompt_embeds is None else _prompt_batch(prompt, prompt_embeds)
        # (PAG first: the other two checks see whether THIS call runs it, not the last one)
        self._pag_call = self._pag_check_call(pag_scale, pag_adaptive_scale, control_image, ip_adapter_image, ip_adapter_image_embeds)
        self._sag_call = self._sag_check_call(sag_scale, guidance_rescale, control_image, ip_adapter_image, ip_adapter_image_embeds)
        self._tgate_check_call(control_image, ip_adapter_image, ip_adapter_image_embeds)
        control = self._control_args(control_image, controlnet_conditioning_scale, control_guidance_start,
                                     control_guidance_end, guess_mode, mask_image, n_prompt)
        a = SimpleNamespace(height=height, width=width, num_inference_steps=num_inference_steps, timesteps=timesteps,
                            sigmas=sigmas, guidance_scale=guidance_scale, negative_prompt=negative_prompt,
                            num_images_per_prompt=num_images_per_prompt, eta=eta, generator=generator, latents=latents,
                            prompt_embeds=prompt_embeds, negative_prompt_embeds=negative_prompt_embeds, output_type=output_type,
                            return_dict=return_dict, guidance_rescale=guidance_rescale, step_noise=step_noise,
                            collect_x0=collect_x0, sample_mode=sample_mode, ip_adapter_image=ip_adapter_image,
                            ip_adapter_image_embeds=ip_adapter_image_embeds, control=control)
        if mask_image is not None:
            if image is None:
                raise ValueError("mask_image without image: inpainting needs the image the mask refers to")
            return self._call_inpaint(prompt, image, mask_image, 1.0 if strength is STRENGTH_UNSET else strength, a)
        if self.unet_config.in_channels == 9:
            raise ValueError("this UNet has 9 input channels (an inpainting checkpoint: latents | mask | masked-image latents): "
                             "it runs only with image= and mask_image=, not as " +
                             ("plain image-to-image" if image is not None else "text-to-image"))
        if image is not None:
            return self._call_img2img(prompt, image, 0.8 if strength is STRENGTH_UNSET else strength, a)
        device, batch_size, do_cfg, ctx = self._begin_call(prompt, height, width, a)
        latents = self._start_loop(batch_size, device, generator, latents, ctx, self._cache_branch(), control)
        return self._run(a, list(self.scheduler._timesteps_list), latents, ctx.shape[0], do_cfg)


# --------------------------------------------------------------------------------------------------
# Variant pipelines: host-only control flow over the same kernels.
# --------------------------------------------------------------------------------------------------
def _lib_dtype_is_fp8(weight_dtype) -> bool:
    from ._lib import DTYPE_FP8_E4M3, DTYPES
    return DTYPES.get(weight_dtype) == DTYPE_FP8_E4M3


def _is_dpm(s) -> bool:
    return hasattr(s, "model_outputs") and hasattr(s, "convert_model_output")


def _push_history(sched, noise_pred, latents):
    """History hand-off (``src/models.py:603-611``, ``:1025-1033``, ``:1045-1053``): shift the other
    scheduler's ``model_outputs`` and append its conversion of this noise prediction.  ``sample=latents``
    is the latents AFTER the step, as the reference writes it."""
    out = sched.convert_model_output(noise_pred, sample=latents)
    model_output = out[0] if isinstance(out, tuple) else out
    for k in range(sched.config.solver_order - 1):
        sched.model_outputs[k] = sched.model_outputs[k + 1]
    sched.model_outputs[-1] = model_output


def _combined(eps, do_cfg, guidance_scale, sched=None):
    """The noise prediction the step saw: CFG combine, scaled by the rescale factors ``sched``'s last step computed
    (``rescale_factors``; None when it did not rescale)."""
    if not do_cfg:
        return eps
    u, c = eps.chunk(2)
    g = u + guidance_scale * (c - u)                                                            # :238-242
    k = getattr(sched, "rescale_factors", None)
    return g if k is None else g * k.view(-1, *([1] * (g.dim() - 1)))


class _VariantBase(StableDiffusionModel):
    """The variants run ``_sample`` over their own list of steps, without DeepCache, and refuse the image arguments."""
    IS_VARIANT = True

    def _refuse_image(self, kwargs):
        if self._sag is not None or kwargs.get("sag_scale") is not None:
            options.check(options.SAG, [options.VARIANT])
        if self._pag is not None or kwargs.get("pag_scale") is not None or kwargs.get("pag_adaptive_scale") is not None:
            options.check(options.PAG, [options.VARIANT])
        if kwargs.get("control_image") is not None or kwargs.get("guess_mode"):
            raise NotImplementedError(f"control_image= (ControlNet) is not built for {type(self).__name__}; "
                                      "StableDiffusionModel runs it")
        if kwargs.get("mask_image") is not None:
            raise NotImplementedError(f"mask_image= (inpainting) is not built for {type(self).__name__}; "
                                      "StableDiffusionModel runs it")
        if kwargs.get("image") is not None:
            raise NotImplementedError(f"image= (image-to-image) is not built for {type(self).__name__}; "
                                      "StableDiffusionModel runs it")

    def _refuse_unipc(self, *schedulers):
        """Before any GPU work: the variants hand a DPM-style history entry from one scheduler to the other (or skip steps
        under a scheduler's feet) and have nothing to give UniPC's ``last_sample``."""
        from .schedulers import UniPCScheduler
        for s in schedulers:
            if isinstance(s, UniPCScheduler):
                raise NotImplementedError(f"UniPCScheduler is not built for {type(self).__name__}: its corrector needs the "
                                          "sample its own previous step corrected, which the hand-off between schedulers "
                                          "(or a skipped step) does not provide; StableDiffusionModel runs it")


@models_registry.add_to_registry("stable_diffusion_model_two_schedulers")
class StableDiffusionModelTwoSchedulers(_VariantBase):
    """``src/models.py:338-730``: ``scheduler_first`` for the first ``num_step_switch`` steps, then
    ``scheduler_second`` from the timestep ``switch_timestamp`` selects.  The second scheduler is handed the
    FIRST scheduler's timesteps as a custom schedule (``:488-492``; ``num_inference_steps_second`` is
    accepted and, as in the reference, not used)."""
    scheduler_first = None
    scheduler_second = None

    @staticmethod
    def switch_timestamp(timesteps_first, timesteps_second, num_step_switch, type_switch="closest"):
        """``src/models.py:704-730``."""
        first = [int(t) for t in timesteps_first][:num_step_switch]
        second = [int(t) for t in timesteps_second]
        pivot = first[-1]
        if type_switch == "closest":
            dist = [abs(t - pivot) for t in second]
            second = second[dist.index(min(dist)):]
        elif type_switch == "left_closest":
            idx = [i for i, t in enumerate(second) if t - pivot >= 0]
            second = second[idx[-1]:]
        elif type_switch == "right_closest":
            idx = [i for i, t in enumerate(second) if t - pivot <= 0]
            second = second[idx[0]:]
        return first, second

    @torch.no_grad()
    def call(self, prompt=None, height=None, width=None, num_inference_steps_first: int = 50,
             num_inference_steps_second: int = 50, num_step_switch: int = 10, type_switch: str = "closest",
             timesteps=None, sigmas=None, guidance_scale: float = 7.5, negative_prompt=None,
             num_images_per_prompt: int = 1, eta: float = 0.0, generator=None, latents=None, prompt_embeds=None,
             negative_prompt_embeds=None, output_type: str = "pil", return_dict: bool = True,
             guidance_rescale: float = 0.0, ip_adapter_image=None, ip_adapter_image_embeds=None, **kwargs):
        self._refuse_image(kwargs)
        if self.scheduler_first is None or self.scheduler_second is None:
            raise ValueError("scheduler_first / scheduler_second must be set (two_schedulers.py:44-62)")
        self._refuse_unipc(self.scheduler_first, self.scheduler_second)
        device, batch_size, do_cfg, ctx = self._begin(prompt, height, width, guidance_scale, negative_prompt,
                                                      num_images_per_prompt, prompt_embeds, negative_prompt_embeds,
                                                      guidance_rescale, timesteps, sigmas, ip_adapter_image, ip_adapter_image_embeds)
        self.scheduler_first.set_timesteps(num_inference_steps_first, device=device)               # :484-487
        self.scheduler_second.set_timesteps(device=device, timesteps=self.scheduler_first._timesteps_list)  # :488-492
        first, second = self.switch_timestamp(self.scheduler_first._timesteps_list,
                                              self.scheduler_second._timesteps_list, num_step_switch, type_switch)
        self.scheduler = self.scheduler_first                     # prepare_latents reads init_noise_sigma
        latents = self._start_loop(batch_size, device, generator, latents, ctx, -1)
        self._num_timesteps = len(first) + len(second)                                              # :545
        hand_off = self.scheduler_second if _is_dpm(self.scheduler_second) else None                # :603-611
        steps = [(t, self.scheduler_first, hand_off) for t in first] + [(t, self.scheduler_second, None) for t in second]  # :550
        latents, x0_preds, execution_time = self._sample(steps, latents, ctx.shape[0], do_cfg, guidance_scale, eta, generator,
                                                         guidance_rescale)
        return self._finish(latents, x0_preds, output_type, return_dict, execution_time)


@models_registry.add_to_registry("stable_diffusion_model_interliving_schedulers")
class StableDiffusionModelInterlivingSchedulers(_VariantBase):
    """``src/models.py:733-1136``: groups of ``solver_order`` steps of ``scheduler_main`` listed in
    ``interliving_steps`` are replaced by one step of ``scheduler_inter`` at the group's first timestep; each
    scheduler's multistep history is fed the other's noise predictions."""
    scheduler_main = None
    scheduler_inter = None

    @staticmethod
    def interleave_plan(timesteps_main, solver_order, interliving_steps):
        """``src/models.py:952-966``: returns (timesteps that run, those of them the inter scheduler takes)."""
        keep, t_inter = [], []
        for i, t in enumerate(int(x) for x in timesteps_main):
            if i // solver_order in interliving_steps:
                if i % solver_order != 0:
                    continue
                t_inter.append(t)
            keep.append(t)
        return keep, t_inter

    @torch.no_grad()
    def call(self, prompt=None, height=None, width=None, num_inference_steps: int = 50, interliving_steps=None,
             timesteps=None, sigmas=None, guidance_scale: float = 7.5, negative_prompt=None,
             num_images_per_prompt: int = 1, eta: float = 0.0, generator=None, latents=None, prompt_embeds=None,
             negative_prompt_embeds=None, output_type: str = "pil", return_dict: bool = True,
             guidance_rescale: float = 0.0, ip_adapter_image=None, ip_adapter_image_embeds=None, **kwargs):
        self._refuse_image(kwargs)
        if self.scheduler_main is None or self.scheduler_inter is None:
            raise ValueError("scheduler_main / scheduler_inter must be set (interliving_exp.py:41-62)")
        self._refuse_unipc(self.scheduler_main, self.scheduler_inter)
        interliving_steps = list(interliving_steps or [])
        device, batch_size, do_cfg, ctx = self._begin(prompt, height, width, guidance_scale, negative_prompt,
                                                      num_images_per_prompt, prompt_embeds, negative_prompt_embeds,
                                                      guidance_rescale, timesteps, sigmas, ip_adapter_image, ip_adapter_image_embeds)
        order = self.scheduler_main.config.solver_order
        self.scheduler_main.set_timesteps(num_inference_steps, device=device)                       # :880-886
        self.scheduler_inter.set_timesteps(num_inference_steps // order, device=device)             # :888-894
        keep, t_inter = self.interleave_plan(self.scheduler_main._timesteps_list, order, interliving_steps)
        self.scheduler = self.scheduler_main
        latents = self._start_loop(batch_size, device, generator, latents, ctx, -1)
        self._num_timesteps = len(self.scheduler_main._timesteps_list) - len(interliving_steps)     # :946
        main, inter = self.scheduler_main, self.scheduler_inter
        to_inter = inter if _is_dpm(inter) else None
        # an inter step feeds the main scheduler's history (:1008-1034), a main step the inter scheduler's (:1035-1054)
        steps = [(t, inter, main) if t in t_inter else (t, main, to_inter) for t in keep]
        latents, x0_preds, execution_time = self._sample(steps, latents, ctx.shape[0], do_cfg, guidance_scale, eta, generator,
                                                         guidance_rescale)
        return self._finish(latents, x0_preds, output_type, return_dict, execution_time)


@models_registry.add_to_registry("stable_diffusion_model_skip_timesteps")
class StableDiffusionModelSkipTimesteps(_VariantBase):
    """``src/models.py:1138-1467``: the plain loop with the loop indices in ``skip_timesteps`` skipped
    (``:1327-1330``).  A multistep scheduler's internal step index is not advanced for a skipped step -- the
    reference's behaviour, kept."""

    @torch.no_grad()
    def call(self, prompt=None, height=None, width=None, num_inference_steps: int = 50, skip_timesteps=None,
             timesteps=None, sigmas=None, guidance_scale: float = 7.5, negative_prompt=None,
             num_images_per_prompt: int = 1, eta: float = 0.0, generator=None, latents=None, prompt_embeds=None,
             negative_prompt_embeds=None, output_type: str = "pil", return_dict: bool = True,
             guidance_rescale: float = 0.0, ip_adapter_image=None, ip_adapter_image_embeds=None, **kwargs):
        self._refuse_image(kwargs)
        self._refuse_unipc(self.scheduler)
        skip = set(int(i) for i in (skip_timesteps or []))
        device, batch_size, do_cfg, ctx = self._begin(prompt, height, width, guidance_scale, negative_prompt,
                                                      num_images_per_prompt, prompt_embeds, negative_prompt_embeds,
                                                      guidance_rescale, timesteps, sigmas, ip_adapter_image, ip_adapter_image_embeds)
        self.scheduler.set_timesteps(num_inference_steps, device=device)
        ts_host = list(self.scheduler._timesteps_list)
        latents = self._start_loop(batch_size, device, generator, latents, ctx, -1)
        self._num_timesteps = len(ts_host)                                                          # :1322
        steps = [(t, self.scheduler, None) for i, t in enumerate(ts_host) if i not in skip]         # :1327-1330
        latents, x0_preds, execution_time = self._sample(steps, latents, ctx.shape[0], do_cfg, guidance_scale, eta, generator,
                                                         guidance_rescale)
        return self._finish(latents, x0_preds, output_type, return_dict, execution_time)


def _fuse_synthetic_lora(sd, seed: int, scale: float, rank: int):
    """``fuse_lora``: W += scale * B @ A on the attention projections (A.6.3).  The LCM-LoRA
    adapter is a network fetch (src/experiments/consistency_model.py:20), so a seeded synthetic
    low-rank update of the same structure is fused instead."""
    g = torch.Generator().manual_seed(seed)
    for name in list(sd.keys()):
        if any(k in name for k in (".to_q.weight", ".to_k.weight", ".to_v.weight", ".to_out.0.weight")):
            w = sd[name]
            o, i = w.shape
            a = torch.randn((rank, i), generator=g) / (i ** 0.5)
            b = torch.randn((o, rank), generator=g) * (0.02 / rank ** 0.5)
            sd[name] = (w + scale * (b @ a)).to(torch.bfloat16).float()
