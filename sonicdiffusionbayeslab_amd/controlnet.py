"""``ControlNetModel``-shaped host object over the libsdhip ControlNet handle (diffusers ``ControlNetModel``, ``guess_mode``
False), and the residual buffer it shares with ``HipUNet2DConditionModel``.

A ControlNet is a second copy of the UNet's encoder that runs at every step: the UNet's time embedding, conv_in (which adds
the step-invariant conditioning embedding in its own launch), down path and mid block on the UNet's kernels, then thirteen
1x1 GEMMs (the zero convs) straight into one caller-owned buffer.  The UNet adds that buffer to its skip tensors and mid
output in one launch (``HipUNet2DConditionModel.set_control_residuals``).  There is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional, Tuple

import torch

from . import _lib
from .handle import HipHandle, Workspace, load_params as _load_params
from .unet import LATENT_CHANNELS, _c_config
from .weights import ControlNetConfig, controlnet_param_shapes, controlnet_residual_shapes


def residual_layout(cfg, unet_batch: int, height: int, width: int) -> Tuple[List[Tuple[int, int, int, int]], int]:
    """([(byte offset, channels, h, w)] of the thirteen segments, total bytes) of the residual buffer at a latent
    ``height`` x ``width``: bf16, channel-last [unet_batch][h * w][C] each, a segment starting where the last one ends rounded
    up to 256 bytes (include/sd_hip.h).  ``cfg``: the UNet's or the ControlNet's config."""
    out, off = [], 0
    for c, h, w in controlnet_residual_shapes(cfg, height, width):
        out.append((off, c, h, w))
        off = (off + unet_batch * h * w * c * 2 + 255) // 256 * 256
    return out, off


def new_residual_buffer(nbytes: int, device) -> torch.Tensor:
    """A 256-byte aligned uint8 view of ``nbytes`` device bytes."""
    ws = Workspace(device)
    ws.reserve(nbytes)
    return ws.view


def unpack_residuals(buf: torch.Tensor, cfg, unet_batch: int, height: int, width: int):
    """The residual buffer -> (twelve down residuals, the mid residual) as NCHW fp32 tensors (tests, diffusers-style calls)."""
    segs, _ = residual_layout(cfg, unet_batch, height, width)
    out = []
    for off, c, h, w in segs:
        n = unet_batch * h * w * c
        out.append(buf[off:off + 2 * n].view(torch.bfloat16).view(unet_batch, h, w, c).permute(0, 3, 1, 2).float())
    return out[:-1], out[-1]


def pack_residuals(down, mid, cfg, device) -> torch.Tensor:
    """diffusers' ``down_block_additional_residuals`` (NCHW float tensors) and ``mid_block_additional_residual`` -> the
    residual buffer (bf16, channel-last): one rounding of the caller's values."""
    res = list(down) + [mid]
    ub, _, height, width = res[0].shape
    segs, total = residual_layout(cfg, ub, height, width)
    if len(res) != len(segs):
        raise ValueError(f"{len(res) - 1} down residuals given, the UNet has {len(segs) - 1} skip tensors")
    buf = new_residual_buffer(total, device)
    for r, (off, c, h, w) in zip(res, segs):
        if tuple(r.shape) != (ub, c, h, w):
            raise ValueError(f"residual of shape {tuple(r.shape)}: expected {(ub, c, h, w)}")
        v = r.detach().to(device, torch.float32).permute(0, 2, 3, 1).contiguous().to(torch.bfloat16)
        buf[off:off + v.numel() * 2].copy_(v.view(-1).view(torch.uint8))
    return buf


def load_params(lib, handle, config: ControlNetConfig, state_dict: Dict[str, torch.Tensor]) -> None:
    _load_params(lib, handle, controlnet_param_shapes(config), state_dict, "ControlNet")


class HipControlNetModel(HipHandle):
    """One ControlNet running on libsdhip.  ``set_context`` (the prompt) and ``set_cond`` (the control image) once per call,
    ``forward_residuals`` once per step."""

    def __init__(self, config: ControlNetConfig, state_dict: Dict[str, torch.Tensor], device: str = "cuda:0",
                 weight_dtype: str = "bf16"):
        if _lib.DTYPES.get(weight_dtype, weight_dtype) != _lib.DTYPE_BF16:
            raise NotImplementedError(f"HipControlNetModel: weight_dtype={weight_dtype!r} is not built (a ControlNet runs in bf16)")
        super().__init__(device)
        self.config = config
        torch.cuda.set_device(self.device)
        ccfg = _c_config(config.unet)
        embed = (C.c_int * 4)(*config.conditioning_embedding_out_channels)
        _lib.check(self._lib.sd_controlnet_create(C.byref(ccfg), embed, C.byref(self._handle)), "sd_controlnet_create")
        load_params(self._lib, self._handle, config, state_dict)
        self._finalize()
        self._ctx_key = None
        self._ctx_keepalive = None
        self._cond_key = None               # (batch, h, w) of the conditioning embedding on the handle
        self._cond_keepalive = None
        self._res: Optional[torch.Tensor] = None
        self._res_key = None
        self._tcond = None

    def latent_size(self, height: Optional[int] = None, width: Optional[int] = None):
        s = self.config.unet.sample_size
        return (s if height is None else int(height)), (s if width is None else int(width))

    def _reserve(self, unet_batch: int, h: int, w: int) -> Workspace:
        key = (unet_batch, h, w)                # (exact key: the context lives in the workspace)
        if not self._wsp.holds(key):
            n = Workspace.bytes_or_raise(self._lib.sd_unet_workspace_bytes_hw(self._handle, unet_batch, -1, h, w),
                                         "sd_unet_workspace_bytes_hw")
            self._wsp.reserve(n, key)
            self._ctx_key = None
        return self._wsp

    def _workspace(self, unet_batch: int, h: int, w: int) -> torch.Tensor:
        return self._reserve(unet_batch, h, w).tensor

    def set_context(self, encoder_hidden_states: torch.Tensor, height: Optional[int] = None, width: Optional[int] = None) -> None:
        """The prompt of the ControlNet's cross-attention layers, as ``HipUNet2DConditionModel.set_context``."""
        h, w = self.latent_size(height, width)
        u = self.config.unet
        ehs = encoder_hidden_states.to(self.device, torch.float32).contiguous()
        if ehs.dim() != 3 or ehs.shape[1] != u.context_len or ehs.shape[2] != u.cross_attention_dim:
            raise ValueError(f"encoder_hidden_states must be [N,{u.context_len},{u.cross_attention_dim}], got {tuple(ehs.shape)}")
        ub = ehs.shape[0]
        ws = self._reserve(ub, h, w)
        _lib.check(self._lib.sd_unet_set_context_hw(self._handle, _lib.current_stream(), ehs.data_ptr(), ub, -1, h, w,
                                                    ws.ptr, ws.nbytes), "sd_unet_set_context_hw")
        self._ctx_keepalive = ehs
        self._ctx_key = (ub, h, w)

    def set_cond(self, cond_image: torch.Tensor) -> None:
        """The control image of a call: ``cond_image`` [Bc,3,8h,8w] floats in [0,1] (rgb, not normalised).  Runs the
        conditioning embedding once and keeps it on the handle; forwards at latent h x w add row ``b % Bc`` to sample b."""
        if not torch.is_tensor(cond_image) or cond_image.dim() != 4 or cond_image.shape[1] != 3 or not cond_image.is_floating_point():
            raise ValueError("cond_image must be a float tensor [B,3,H,W] in [0,1]")
        b, _, hh, ww = cond_image.shape
        if hh % 8 or ww % 8:
            raise ValueError(f"cond_image {hh}x{ww}: sides must be 8 x the latent's")
        img = cond_image.detach().to(self.device, torch.float32).contiguous()
        if img.data_ptr() % 16:
            img = img.clone()
        _lib.check(self._lib.sd_controlnet_set_cond_hw(self._handle, _lib.current_stream(), img.data_ptr(), b, hh // 8, ww // 8),
                   "sd_controlnet_set_cond_hw")
        self._cond_keepalive = img
        self._cond_key = (b, hh // 8, ww // 8)

    def set_timestep_cond(self, cond: Optional[torch.Tensor]) -> None:
        """Condition of a ControlNet whose time embedding has a ``cond_proj`` (``config.unet.time_cond_proj_dim``), as
        ``HipUNet2DConditionModel.set_timestep_cond``; None clears it.  (diffusers' pipeline passes a ControlNet no
        ``timestep_cond``; ``ControlNetModel.forward`` takes one.)"""
        if cond is None:
            _lib.check(self._lib.sd_unet_set_timestep_cond(self._handle, _lib.current_stream(), None), "sd_unet_set_timestep_cond")
            self._tcond = None
            return
        d = self.config.unet.time_cond_proj_dim
        if d is None:
            raise ValueError("timestep_cond given, but this ControlNet has no time_embedding.cond_proj (time_cond_proj_dim is None)")
        row = cond.detach().to(self.device, torch.float32).reshape(-1).contiguous()
        if row.numel() != d:
            raise ValueError(f"timestep_cond must be [{d}] or [1, {d}], got {tuple(cond.shape)}")
        if row.data_ptr() % 16:
            row = row.clone()
        _lib.check(self._lib.sd_unet_set_timestep_cond(self._handle, _lib.current_stream(), row.data_ptr()), "sd_unet_set_timestep_cond")
        self._tcond = row                   # (keeps the operand alive until the GEMV has run)

    def clear_cond(self) -> None:
        _lib.check(self._lib.sd_controlnet_set_cond_hw(self._handle, _lib.current_stream(), None, 0, 0, 0), "sd_controlnet_set_cond_hw")
        self._cond_key = None
        self._cond_keepalive = None

    def residual_buffer(self, unet_batch: int, h: int, w: int) -> torch.Tensor:
        key = (unet_batch, h, w)
        if self._res is None or self._res_key != key:
            n = Workspace.bytes_or_raise(self._lib.sd_controlnet_residual_bytes_hw(self._handle, unet_batch, h, w),
                                         "sd_controlnet_residual_bytes_hw")
            assert n == residual_layout(self.config, unet_batch, h, w)[1]
            self._res = None
            self._res = new_residual_buffer(n, self.device)
            self._res_key = key
        return self._res

    def forward_residuals(self, latents: torch.Tensor, unet_batch: int, timestep: float,
                          out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The thirteen residuals (unscaled) of fp32 NCHW ``latents`` [B,4,h,w] into the residual buffer (``out`` or the
        model's own, reused from step to step); ``unet_batch`` is B or 2 B (CFG: the duplication is fused).  ``set_context``
        and ``set_cond`` must have run for this batch and size."""
        if latents.dim() != 4 or latents.shape[1] != LATENT_CHANNELS:
            raise ValueError(f"latents must be [B,{LATENT_CHANNELS},H,W], got {tuple(latents.shape)}")
        b, _, h, w = latents.shape
        if self._ctx_key != (unet_batch, h, w):
            raise _lib.SdHipError(f"set_context(encoder_hidden_states, {h}, {w}) must be called for this batch ({unet_batch}) and size first")
        if self._cond_key is None or self._cond_key[1:] != (h, w) or b % self._cond_key[0]:
            raise _lib.SdHipError(f"set_cond(cond_image) must be called for this size ({8 * h}x{8 * w} pixels) and a batch dividing {b} first")
        if latents.dtype != torch.float32 or not latents.is_contiguous() or latents.device != self.device:
            latents = latents.to(self.device, torch.float32).contiguous()
        buf = self.residual_buffer(unet_batch, h, w) if out is None else out
        ws = self._reserve(unet_batch, h, w)
        _lib.check(self._lib.sd_controlnet_forward_hw(self._handle, _lib.current_stream(), latents.data_ptr(), b, unet_batch, h, w,
                                                      float(timestep), buf.data_ptr(), ws.ptr, ws.nbytes),
                   "sd_controlnet_forward_hw")
        return buf

    def __call__(self, sample: torch.Tensor, timestep, encoder_hidden_states: torch.Tensor, controlnet_cond: torch.Tensor,
                 conditioning_scale: float = 1.0, guess_mode: bool = False, return_dict: bool = False, **kwargs):
        """diffusers-style call: (down_block_res_samples, mid_block_res_sample) as NCHW tensors times ``conditioning_scale``."""
        if guess_mode:
            raise NotImplementedError("guess_mode is not built")
        if isinstance(conditioning_scale, (list, tuple)):
            raise NotImplementedError("a list of conditioning scales (Multi-ControlNet) is not built")
        h, w = sample.shape[2], sample.shape[3]
        self.set_context(encoder_hidden_states, h, w)
        self.set_cond(controlnet_cond)
        t = float(timestep.item()) if torch.is_tensor(timestep) else float(timestep)
        buf = self.forward_residuals(sample, sample.shape[0], t)
        down, mid = unpack_residuals(buf, self.config, sample.shape[0], h, w)
        s = float(conditioning_scale)
        return [d * s for d in down], mid * s

    def debug_cond_embedding(self) -> torch.Tensor:
        """The stored conditioning embedding [Bc, h, w, C] as fp32 on the host (handles created with SD_DEBUG_TAPS=1)."""
        b, h, w = self._cond_key
        c = self.config.unet.block_out_channels[0]
        out = torch.empty(b * h * w * c, dtype=torch.float32)
        _lib.check(self._lib.sd_unet_debug_tensor(self._handle, _lib.current_stream(), b"cond_embedding", out.data_ptr(), out.numel(),
                                                  None, b, -1), "sd_unet_debug_tensor")
        return out.view(b, h, w, c)
