"""``UNet2DConditionModel``-shaped host object over the libsdhip UNet handle.

Replaces ``pipe.unet`` of the reference pipeline: the call
``self.unet(latent_model_input, t, encoder_hidden_states=prompt_embeds, ...)[0]``
(``src/models.py:227-235``) works unchanged, and the sampling loop additionally uses
``forward_latents`` which fuses the CFG duplication ``torch.cat([latents]*2)``
(``src/models.py:217``) into conv_in.  All arithmetic runs in hand-written gfx950 kernels; torch
only owns the device buffers.  There is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Dict, Optional

import torch

from . import _lib, options
from .handle import ALIGN, HipHandle, Workspace, load_params as _load_params
from .weights import UNetConfig, param_shapes

CACHE_OFF, CACHE_FULL_AND_STORE, CACHE_SKIP = 0, 1, 2
LATENT_CHANNELS = 4         # channels of the latents crossing the ABI (an inpainting UNet's other 5 are set per call)


def _c_config(cfg: UNetConfig, weight_dtype: str = "bf16", fp8_act_scales=(0.0, 0.0)) -> _lib.SdUnetConfigFull:
    c = _lib.SdUnetConfigFull()
    if weight_dtype not in _lib.DTYPES:
        raise ValueError(f"weight_dtype {weight_dtype!r}: one of {sorted(_lib.DTYPES)}")
    c.weight_dtype = _lib.DTYPES[weight_dtype]
    c.fp8_act_scale_norm, c.fp8_act_scale_ff = float(fp8_act_scales[0]), float(fp8_act_scales[1])
    c.sample_size, c.in_channels, c.out_channels = cfg.sample_size, cfg.in_channels, cfg.out_channels
    c.num_levels = len(cfg.block_out_channels)
    for i, v in enumerate(cfg.block_out_channels):
        c.block_out_channels[i] = v
        c.attn_levels[i] = int(cfg.attn_levels[i])
    c.layers_per_block = cfg.layers_per_block
    c.cross_attention_dim, c.num_heads = cfg.cross_attention_dim, cfg.num_heads
    c.norm_num_groups, c.norm_eps, c.context_len = cfg.norm_num_groups, cfg.norm_eps, cfg.context_len
    c.time_cond_proj_dim = cfg.time_cond_proj_dim or 0
    c.ip_adapter_tokens, c.ip_adapter_embed_dim = cfg.ip_adapter_tokens or 0, cfg.ip_adapter_embed_dim or 0
    for i, v in enumerate(cfg.num_heads_per_level or ()):       # (None: all zeros = num_heads at every level)
        c.num_heads_per_level[i] = int(v)
    return c


def load_params(lib, handle, config: UNetConfig, state_dict: Dict[str, torch.Tensor]) -> None:
    """Every parameter ``param_shapes(config)`` names, checked for presence and shape, into the handle
    (``sd_unet_load_param`` copies; host-only, runs without a GPU).  Tensors of any float dtype are accepted --
    diffusers checkpoints are fp16 on disk."""
    _load_params(lib, handle, param_shapes(config), state_dict, "UNet")


class HipUNet2DConditionModel(HipHandle):
    """SD-1.5 UNet running on libsdhip.  ``config`` mirrors the diffusers attributes the
    reference loop reads (``in_channels``, ``sample_size``, ``time_cond_proj_dim``)."""

    def __init__(self, config: UNetConfig, state_dict: Dict[str, torch.Tensor], device: str = "cuda:0",
                 weight_dtype: str = "bf16", fp8_act_scales=(0.0, 0.0)):
        """``weight_dtype="fp8"``: OCP e4m3 weights (per-output-channel scales) and e4m3 activations with static
        per-tensor scales for the resnet 3x3 convs, proj_in, the self-attention QKV projection and the feed-forward
        GEMMs (include/sd_hip.h::sd_unet_config.weight_dtype; BASELINE configs[4])."""
        super().__init__(device)
        self.config = config
        self.dtype = torch.float32          # dtype of latents / eps crossing the ABI
        torch.cuda.set_device(self.device)
        self.weight_dtype = "fp8_e4m3" if _lib.DTYPES.get(weight_dtype) == _lib.DTYPE_FP8_E4M3 else "bf16"
        ccfg = _c_config(config, weight_dtype, fp8_act_scales)
        _lib.check(self._lib.sd_unet_create(C.byref(ccfg), C.byref(self._handle)), "sd_unet_create")
        load_params(self._lib, self._handle, config, state_dict)
        self._finalize()
        self._ctx_key = None
        self._ctx_keepalive = None
        self._cond = None                   # the condition set on the handle (device fp32 [time_cond_proj_dim]) or None
        self._inpaint_key = None            # (batch, h, w) of the inpainting condition on the handle (in_channels == 9)
        # IP-Adapter image prompt (config.ip_adapter_embed_dim set): _ip_on = forwards run with one; _ip_keys = the (batch,
        # branch, h, w) whose workspace holds folded image operands; _ip_call = what __call__ last set (embeds identity, scale)
        self._ip_on = False
        self._ip_keys = set()
        self._ip_call = None
        self._ip_keepalive = None
        self.ip_adapter_scale = 1.0         # scale __call__(added_cond_kwargs=...) applies (diffusers: set_ip_adapter_scale)
        # ControlNet residuals on the handle: (buffer kept alive, scale, unet batch, h, w) or None (the plain plans)
        self._control = None
        self._tome = None                   # (ratio, max_downsample) of the Token Merging setting on the handle, None = off
        self._tome_choice_keepalive = None
        self._freeu = None                  # (s1, s2, b1, b2) on the handle, None = off
        self._hypertile = None              # (tile_tokens, max_depth) of the HyperTile setting on the handle, None = off
        self._pag = 0                       # the PAG layer mask on the handle, 0 = off
        # SAG: _sag = capture of the mid block's attention mass is on; _sag_mass = the fp32 buffer the handle writes it to;
        # _sag_ws = the workspace of the SAG forward (the degraded latents at the latent batch, capture off) with its own prompt
        # context, keyed (batch, h, w): the main workspace keeps the context of the first forward
        self._sag = False
        self._sag_mass = None
        self._sag_ws = Workspace(self.device)
        self._sag_ctx_key = None
        # T-GATE: _tgate = (mode, latent batch, h, w) on the handle or None = off; _tgate_cache = the buffer the handle borrows;
        # _tgate_ws = workspace of the gated (reuse) plans, keyed (batch, h, w): the main workspace keeps the prompt context
        self._tgate = None
        self._tgate_cache = Workspace(self.device)
        self._tgate_ws = Workspace(self.device)
        self._tgate_reserve = None          # (latent batch, h, w): _workspace also covers the capture plans of that layout
        self.cache_branch_id = -1

    # -- workspace / context ---------------------------------------------------------------
    # Every setting that changes the plans drops the main workspace's key (``self._ws_key = None``).  The workspace of the SAG
    # forward was sized and laid out for the plans of the old setting as well, so it goes with it: the next ``set_sag_context``
    # sizes a new one and folds its context again.
    @property
    def _ws_key(self):
        return self._wsp.key

    @_ws_key.setter
    def _ws_key(self, key) -> None:
        self._wsp.key = key
        if key is None and getattr(self, "_sag_ws", None) is not None:
            self._sag_ws.key = None
            self._sag_ctx_key = None

    def options_on(self) -> list:
        """The options on this handle now (``options.HANDLE_OPTIONS``): what every setter checks the one it is asked for against."""
        state = ((options.DEEPCACHE, self.cache_branch_id != -1), (options.IP_PROMPT, self._ip_on),
                 (options.CONTROL, self._control is not None), (options.TOME, self._tome is not None),
                 (options.HYPERTILE, self._hypertile is not None), (options.FREEU, self._freeu is not None),
                 (options.TGATE, self._tgate is not None), (options.PAG, bool(self._pag)), (options.SAG, self._sag))
        return options.handle_options(self.config, self.weight_dtype) + [name for name, on in state if on]

    def _check_option(self, asked: str) -> None:
        options.check(asked, self.options_on(), options.HANDLE_OFF)

    def latent_size(self, height: Optional[int] = None, width: Optional[int] = None):
        """(h, w) of the latent: ``sample_size`` where not given."""
        s = self.config.sample_size
        return (s if height is None else int(height)), (s if width is None else int(width))

    def _workspace_bytes(self, unet_batch: int, branch: int, h: int, w: int) -> int:
        return Workspace.bytes_or_raise(self._lib.sd_unet_workspace_bytes_hw(self._handle, unet_batch, branch, h, w),
                                        "sd_unet_workspace_bytes_hw")

    def _reserve(self, unet_batch: int, h: Optional[int] = None, w: Optional[int] = None) -> Workspace:
        """The main workspace for this batch, DeepCache branch and size (exact key: the context lives in it)."""
        h, w = self.latent_size(h, w)
        key = (unet_batch, self.cache_branch_id, h, w)
        if not self._wsp.holds(key):
            n = self._workspace_bytes(unet_batch, self.cache_branch_id, h, w)
            if self._tgate_reserve is not None and self._tgate_reserve[1:] == (h, w) and self._tgate is None:
                n = max(n, self._tgate_capture_bytes(unet_batch, *self._tgate_reserve))
            self._drop_ip_keys()            # (the folded image operands lived in the old workspace, like the context)
            self._wsp.reserve(n, key)
            self._ctx_key = None
        return self._wsp

    def _workspace(self, unet_batch: int, h: Optional[int] = None, w: Optional[int] = None) -> torch.Tensor:
        return self._reserve(unet_batch, h, w).tensor

    def set_deepcache(self, cache_branch_id: int) -> None:
        """-1 disables the DeepCache plan; >= 0 reserves that branch's cached tensors."""
        if cache_branch_id != -1:
            self._check_option(options.DEEPCACHE)
        if cache_branch_id != self.cache_branch_id:
            self.cache_branch_id = cache_branch_id
            self._ws_key = None

    def set_context(self, encoder_hidden_states: torch.Tensor, height: Optional[int] = None,
                    width: Optional[int] = None) -> None:
        """Project K/V of the prompt for all cross-attention layers (once per sampling run), for forwards at latent
        ``height`` x ``width`` (default ``sample_size``; a forward at another size needs a new ``set_context``)."""
        h, w = self.latent_size(height, width)
        ehs = encoder_hidden_states.to(self.device, torch.float32).contiguous()
        ub = ehs.shape[0]
        if ehs.shape[1] != self.config.context_len or ehs.shape[2] != self.config.cross_attention_dim:
            raise ValueError(f"encoder_hidden_states must be [N,{self.config.context_len},"
                             f"{self.config.cross_attention_dim}], got {tuple(ehs.shape)}")
        ws = self._reserve(ub, h, w)
        _lib.check(self._lib.sd_unet_set_context_hw(self._handle, _lib.current_stream(), ehs.data_ptr(), ub,
                                                    self.cache_branch_id, h, w, ws.ptr, ws.nbytes),
                   "sd_unet_set_context_hw")
        self._ctx_keepalive = ehs
        self._ctx_key = (encoder_hidden_states.data_ptr(), encoder_hidden_states._version, ub, h, w)

    def set_timestep_cond(self, cond: Optional[torch.Tensor]) -> None:
        """Condition of an LCM-distilled UNet (``time_cond_proj_dim`` set): ``cond`` [d] or [1, d], e.g.
        ``get_guidance_scale_embedding(guidance_scale - 1, d)``.  Every later forward adds ``cond_proj(cond)`` to its timestep
        sinusoid (one GEMV now, none per forward).  ``None`` clears it: forwards then skip the projection, as diffusers does
        for ``timestep_cond=None``."""
        if cond is None:
            _lib.check(self._lib.sd_unet_set_timestep_cond(self._handle, _lib.current_stream(), None), "sd_unet_set_timestep_cond")
            self._cond = None
            return
        d = self.config.time_cond_proj_dim
        if d is None:
            raise ValueError("timestep_cond given, but this UNet has no time_embedding.cond_proj (time_cond_proj_dim is None)")
        row = cond.detach().to(self.device, torch.float32).reshape(-1).contiguous()
        if row.numel() != d:
            raise ValueError(f"timestep_cond must be [{d}] or [1, {d}], got {tuple(cond.shape)}")
        if row.data_ptr() % 16:
            row = row.clone()
        _lib.check(self._lib.sd_unet_set_timestep_cond(self._handle, _lib.current_stream(), row.data_ptr()),
                   "sd_unet_set_timestep_cond")
        self._cond = row                    # (also keeps the operand alive until the GEMV has run)

    def set_inpaint_cond(self, mask: torch.Tensor, masked_latents: torch.Tensor) -> None:
        """Condition of an inpainting UNet (``in_channels == 9``): ``mask`` [B,1,h,w] (0 / 1, 1 = repaint) and
        ``masked_latents`` [B,4,h,w] (scaled encoding of the masked image), stored on the handle once per call (one launch);
        every later forward at this size reads them as input channels 4..8, duplicated under CFG like the latents."""
        if self.config.in_channels != 9:
            raise ValueError(f"set_inpaint_cond: this UNet has in_channels = {self.config.in_channels} (an inpainting UNet has 9)")
        m = mask.detach().to(self.device, torch.float32).contiguous()
        z = masked_latents.detach().to(self.device, torch.float32).contiguous()
        if m.dim() != 4 or z.dim() != 4 or m.shape[1] != 1 or z.shape[1] != LATENT_CHANNELS or m.shape[0] != z.shape[0] \
                or m.shape[2:] != z.shape[2:]:
            raise ValueError(f"set_inpaint_cond: mask [B,1,h,w] and masked_latents [B,{LATENT_CHANNELS},h,w], got "
                             f"{tuple(m.shape)} and {tuple(z.shape)}")
        b, _, h, w = z.shape
        _lib.check(self._lib.sd_unet_set_inpaint_cond_hw(self._handle, _lib.current_stream(), m.data_ptr(), z.data_ptr(), b, h, w),
                   "sd_unet_set_inpaint_cond_hw")
        self._inpaint_key = (b, h, w)

    def clear_inpaint_cond(self) -> None:
        """Drop the inpainting condition of the handle: the next forward needs a ``set_inpaint_cond`` of its own."""
        _lib.check(self._lib.sd_unet_set_inpaint_cond_hw(self._handle, _lib.current_stream(), None, None, 0, 0, 0),
                   "sd_unet_set_inpaint_cond_hw")
        self._inpaint_key = None

    # -- IP-Adapter image prompt ---------------------------------------------------------------
    def _drop_ip_keys(self) -> None:
        for ub, branch, h, w in self._ip_keys:
            _lib.check(self._lib.sd_unet_set_ip_adapter_hw(self._handle, _lib.current_stream(), None, ub, branch, h, w, 0.0, None, 0),
                       "sd_unet_set_ip_adapter_hw")
        self._ip_keys = set()
        self._ip_call = None

    def set_ip_adapter(self, image_embeds: torch.Tensor, scale: float = 1.0, height: Optional[int] = None,
                       width: Optional[int] = None) -> None:
        """Image prompt of a UNet built with an IP-Adapter: ``image_embeds`` [N, E] fp32 (N = the UNet batch, CFG halves
        already concatenated, negative first) for forwards at latent ``height`` x ``width``.  Call it after ``set_context``
        for the same batch and size: it projects the image tokens, ``to_k_ip`` / ``to_v_ip`` of every attn2 layer and folds
        them with ``scale`` into per-sample operands in the workspace (once per sampling run; a new scale means a new call).
        Every later forward adds ``scale * softmax(q K_ip^T / sqrt d) V_ip`` to its prompt cross-attention until
        ``clear_ip_adapter``."""
        e = self.config.ip_adapter_embed_dim
        if e is None:
            raise ValueError("set_ip_adapter: this UNet was built without an IP-Adapter (ip_adapter_embed_dim is None)")
        if isinstance(scale, dict) or not isinstance(scale, (int, float)) or isinstance(scale, bool):
            raise NotImplementedError("set_ip_adapter: scale must be one float (per-block scale dicts are not built)")
        if not torch.is_tensor(image_embeds) or image_embeds.dim() != 2 or image_embeds.shape[1] != e:
            raise ValueError(f"image_embeds must be [N, {e}], got "
                             f"{tuple(image_embeds.shape) if torch.is_tensor(image_embeds) else type(image_embeds).__name__}")
        h, w = self.latent_size(height, width)
        ub = int(image_embeds.shape[0])
        if self._ctx_key is None or self._ctx_key[2:] != (ub, h, w):
            raise _lib.SdHipError(f"set_context(encoder_hidden_states, {h}, {w}) must be called for this batch ({ub}) and size first")
        emb = image_embeds.detach().to(self.device, torch.float32).contiguous()
        if emb.data_ptr() % 16:
            emb = emb.clone()
        ws = self._reserve(ub, h, w)
        _lib.check(self._lib.sd_unet_set_ip_adapter_hw(self._handle, _lib.current_stream(), emb.data_ptr(), ub, self.cache_branch_id,
                                                       h, w, float(scale), ws.ptr, ws.nbytes),
                   "sd_unet_set_ip_adapter_hw")
        self._ip_keepalive = emb
        self._ip_keys.add((ub, self.cache_branch_id, h, w))
        self._ip_on = True

    def clear_ip_adapter(self) -> None:
        """Drop every image prompt of the handle: forwards are again those of a UNet without an adapter, bit for bit."""
        self._drop_ip_keys()
        self._ip_on = False
        self._ip_keepalive = None

    # -- ControlNet residuals ---------------------------------------------------------------------
    def set_control_residuals(self, residuals: torch.Tensor, scale: float, unet_batch: int, height: Optional[int] = None,
                              width: Optional[int] = None) -> None:
        """``residuals``: the buffer ``HipControlNetModel.forward_residuals`` fills (bf16, channel-last, thirteen segments;
        ``controlnet.residual_layout``) for forwards of ``unet_batch`` at latent ``height`` x ``width``.  Every later forward
        adds ``scale`` times the residuals to its twelve skip tensors and its mid block's output, in one launch after the mid
        block, until ``clear_control_residuals``.  The buffer is borrowed: the ControlNet may refill it before every step."""
        from .controlnet import residual_layout
        self._check_option(options.CONTROL)
        h, w = self.latent_size(height, width)
        need = residual_layout(self.config, unet_batch, h, w)[1]
        if not torch.is_tensor(residuals) or residuals.dtype != torch.uint8 or residuals.device != self.device or \
                residuals.numel() < need or residuals.data_ptr() % ALIGN:
            raise ValueError(f"residuals must be a {ALIGN}-byte aligned uint8 device tensor of at least {need} bytes "
                             "(controlnet.new_residual_buffer)")
        _lib.check(self._lib.sd_unet_set_control_residuals_hw(self._handle, residuals.data_ptr(), float(scale), unet_batch, h, w),
                   "sd_unet_set_control_residuals_hw")
        self._control = (residuals, float(scale), unet_batch, h, w)
        self._grow_workspace_for_control()

    def _grow_workspace_for_control(self) -> None:
        """The handle sizes the control plan variants only once residuals were set on it: if the live workspace is smaller
        than they need, move it into a larger one.  The context tensors (prompt, image prompt) lie at the same offsets in
        every variant, at the front of the workspace, so the copy keeps them."""
        old = self._wsp
        if old.tensor is None or old.key is None:       # (no key: the next _workspace sizes a new one anyway)
            return
        n = self._workspace_bytes(*old.key)
        if n > old.nbytes:
            self._wsp = Workspace(self.device)
            self._wsp.reserve(n, old.key)
            self._wsp.view[:old.nbytes].copy_(old.view)

    def clear_control_residuals(self) -> None:
        """Forwards are again those of a UNet that never saw a ControlNet, bit for bit."""
        if self._control is not None:
            _lib.check(self._lib.sd_unet_set_control_residuals_hw(self._handle, None, 0.0, 0, 0, 0), "sd_unet_set_control_residuals_hw")
            self._control = None

    # -- Token Merging (include/sd_hip.h::sd_unet_set_tome) -----------------------------------------
    def set_tome(self, ratio: float, max_downsample: int = 1) -> None:
        """Merge ``r = min(num_src, int(tokens * ratio))`` src tokens around the self-attention of every transformer block
        whose level is at most ``max_downsample`` times coarser than the latent (``ratio`` 0: off, the handle of before).  A
        change needs a new workspace and a new ``set_context``; both follow from dropping the workspace key here."""
        ratio = float(ratio)
        if ratio > 0.0:
            self._check_option(options.TOME)
        _lib.check(self._lib.sd_unet_set_tome(self._handle, ratio, int(max_downsample) if ratio > 0.0 else 0), "sd_unet_set_tome")
        new = (ratio, int(max_downsample)) if ratio > 0.0 else None
        if new != self._tome:
            self._tome = new
            self._ws_key = None
            self._tome_choice_keepalive = None

    def tome_blocks(self, height: Optional[int] = None, width: Optional[int] = None):
        """The merging blocks at a latent size, in plan order: dicts of ``h``, ``w`` (token grid), ``r`` and ``choice_off``
        (where the block's ``h/2 * w/2`` choice bytes start in the array of ``set_tome_choice``).  Empty while off."""
        lh, lw = self.latent_size(height, width)
        n = self._lib.sd_unet_tome_block_count_hw(self._handle, lh, lw)
        if n < 0:
            _lib.check(-1, "sd_unet_tome_block_count_hw")
        out = []
        for i in range(n):
            h, w, r, off = C.c_int(), C.c_int(), C.c_int(), C.c_longlong()
            _lib.check(self._lib.sd_unet_tome_block_info_hw(self._handle, i, lh, lw, C.byref(h), C.byref(w), C.byref(r), C.byref(off)),
                       "sd_unet_tome_block_info_hw")
            out.append(dict(h=h.value, w=w.value, r=r.value, choice_off=off.value))
        return out

    def set_tome_choice(self, choice: torch.Tensor, height: Optional[int] = None, width: Optional[int] = None) -> None:
        """``choice``: uint8, the dst position (0..3) of every 2x2 cell of every merging block, concatenated in plan order
        (``tome_blocks``); one asynchronous copy on the current stream.  A host tensor should be pinned and is kept alive until
        the next call."""
        lh, lw = self.latent_size(height, width)
        if not torch.is_tensor(choice) or choice.dtype != torch.uint8 or choice.dim() != 1 or not choice.is_contiguous():
            raise ValueError("choice must be a contiguous 1-D uint8 tensor")
        _lib.check(self._lib.sd_unet_set_tome_choice_hw(self._handle, _lib.current_stream(), choice.data_ptr(), choice.numel(), lh, lw),
                   "sd_unet_set_tome_choice_hw")
        self._tome_choice_keepalive = choice

    def tome_matching(self, block: int, unet_batch: int, height: Optional[int] = None, width: Optional[int] = None):
        """What the last forward matched in merging block ``block``: dict of int32 CPU tensors ``kept`` [B, num_src - r],
        ``merged`` [B, r], ``dst_idx`` [B, r] (src / dst slot numbers), ``tok`` [h * w] (token index of every src slot, then
        of every dst slot) and ``r``; B is half the UNet batch for the first block of a CFG pair.  Synchronises."""
        lh, lw = self.latent_size(height, width)
        info = self.tome_blocks(lh, lw)[block]
        n = info["h"] * info["w"]
        num_src, r = n - n // 4, info["r"]
        kept = torch.full((unet_batch, num_src - r), -1, dtype=torch.int32)
        merged = torch.full((unet_batch, r), -1, dtype=torch.int32)
        dst_idx = torch.full((unet_batch, r), -1, dtype=torch.int32)
        tok = torch.full((n,), -1, dtype=torch.int32)
        rr, bb = C.c_int(), C.c_int()
        ws = self._reserve(unet_batch, lh, lw)
        _lib.check(self._lib.sd_unet_tome_matching_hw(self._handle, _lib.current_stream(), block, unet_batch, self.cache_branch_id,
                                                      ws.ptr, kept.data_ptr(), merged.data_ptr(), dst_idx.data_ptr(),
                                                      tok.data_ptr(), C.byref(rr), C.byref(bb)), "sd_unet_tome_matching_hw")
        b = bb.value
        # (the library wrote B rows contiguously at the row lengths above)
        return dict(kept=kept.reshape(-1)[:b * (num_src - r)].reshape(b, num_src - r), merged=merged.reshape(-1)[:b * r].reshape(b, r),
                    dst_idx=dst_idx.reshape(-1)[:b * r].reshape(b, r), tok=tok, r=rr.value)

    # -- HyperTile (include/sd_hip.h::sd_unet_set_hypertile) -----------------------------------------
    HYPERTILE_MIN_TOKENS = 8

    @staticmethod
    def check_hypertile_args(tile_tokens, max_depth, weight_dtype="bf16"):
        """The arguments of ``set_hypertile`` checked, by name, without touching the GPU; returns ``(tile_tokens, max_depth)``
        as ints, or None for ``tile_tokens == 0`` (off)."""
        if isinstance(tile_tokens, bool) or not isinstance(tile_tokens, int) or \
                (tile_tokens != 0 and not HipUNet2DConditionModel.HYPERTILE_MIN_TOKENS <= tile_tokens <= 256):
            raise ValueError(f"tile_tokens={tile_tokens!r}: the HyperTile tile side is an integer of 8 .. 256 tokens (0 = off)")
        if tile_tokens == 0:
            return None
        if isinstance(max_depth, bool) or not isinstance(max_depth, int) or not 0 <= max_depth <= 3:
            raise ValueError(f"max_depth={max_depth!r}: HyperTile takes an integer max_depth of 0 .. 3")
        options.check(options.HYPERTILE, options.handle_options(None, weight_dtype))
        return tile_tokens, max_depth

    def set_hypertile(self, tile_tokens: int, max_depth: int = 0) -> None:
        """Tiled self-attention (HyperTile): every transformer block at depth ``<= max_depth`` whose token grid is cut into
        more than one tile -- the tile side is the smallest divisor of the grid's side that is ``>= min(tile_tokens, side)`` --
        runs in tile order, its self-attention inside each tile (``tile_tokens`` 0: off, the handle of before).  A change needs a new workspace and a new ``set_context``; both follow
        from dropping the workspace key here.  Refused together with Token Merging."""
        new = self.check_hypertile_args(tile_tokens, max_depth, self.weight_dtype)
        if new is not None:
            self._check_option(options.HYPERTILE)
        _lib.check(self._lib.sd_unet_set_hypertile(self._handle, *(new or (0, 0))), "sd_unet_set_hypertile")
        if new != self._hypertile:
            self._hypertile = new
            self._ws_key = None
            self._tgate_ws.clear()          # (the gated plans of the other setting sized it)

    def hypertile_blocks(self, height: Optional[int] = None, width: Optional[int] = None):
        """The tiled blocks at a latent size, in plan order (down, mid, up): dicts of ``rh``, ``rw`` (token grid) and ``nh``,
        ``nw`` (tile counts).  Empty while off."""
        lh, lw = self.latent_size(height, width)
        n = self._lib.sd_unet_hypertile_block_count_hw(self._handle, lh, lw)
        if n < 0:
            _lib.check(-1, "sd_unet_hypertile_block_count_hw")
        out = []
        for i in range(n):
            v = [C.c_int() for _ in range(4)]
            _lib.check(self._lib.sd_unet_hypertile_block_info_hw(self._handle, i, lh, lw, *[C.byref(x) for x in v]),
                       "sd_unet_hypertile_block_info_hw")
            out.append(dict(rh=v[0].value, rw=v[1].value, nh=v[2].value, nw=v[3].value))
        return out

    # -- PAG (include/sd_hip.h::sd_unet_set_pag) --------------------------------------------------------
    @staticmethod
    def pag_block_names(config) -> list:
        """The transformer blocks of a UNet in plan order (down, mid, up), as diffusers' ``pag_applied_layers`` spells them:
        ``down.block_i.attentions_j``, ``mid``, ``up.block_i.attentions_j``.  Bit ``k`` of a PAG layer mask is entry ``k``."""
        nl = len(config.block_out_channels)
        out = []
        for i in range(nl):
            if config.attn_levels[i]:
                out += [f"down.block_{i}.attentions_{j}" for j in range(config.layers_per_block)]
        out.append("mid")
        for i in range(nl):
            if config.attn_levels[nl - 1 - i]:
                out += [f"up.block_{i}.attentions_{j}" for j in range(config.layers_per_block + 1)]
        return out

    @classmethod
    def pag_layer_mask(cls, config, applied_layers) -> int:
        """``pag_applied_layers`` -> the layer mask of ``set_pag``.  A name is ``"mid"``, ``"down.block_i"`` / ``"up.block_i"``
        (every transformer block of that block) or ``"down.block_i.attentions_j"`` / ``"up.block_i.attentions_j"``; a string or a
        list of them.  A name that matches no transformer block is a ``ValueError`` that lists the valid names."""
        blocks = cls.pag_block_names(config)
        groups = sorted({b.rsplit(".attentions_", 1)[0] for b in blocks if b != "mid"})
        names = [applied_layers] if isinstance(applied_layers, str) else list(applied_layers)
        if not names:
            raise ValueError(f"pag_applied_layers is empty; valid names: {groups + blocks}")
        mask = 0
        for name in names:
            hit = [k for k, b in enumerate(blocks) if isinstance(name, str) and (b == name or b.startswith(name + ".attentions_"))]
            if not hit:
                raise ValueError(f"pag_applied_layers: {name!r} matches no transformer block of this UNet; valid names: "
                                 f"{groups + blocks}")
            for k in hit:
                mask |= 1 << k
        return mask

    @staticmethod
    def check_pag_handle(config, weight_dtype="bf16"):
        """What ``set_pag`` refuses about the handle, by name, without touching the GPU."""
        options.check(options.PAG, options.handle_options(config, weight_dtype))

    def set_pag(self, layer_mask: int) -> None:
        """Perturbed-attention guidance: bit ``k`` of ``layer_mask`` = transformer block ``k`` in plan order
        (``pag_block_names``) replaces the self-attention of the LAST third (or half) of the UNet batch by the identity; 0 =
        off, the handle of before.  Forwards then take a UNet batch of 3 or 2 times the latent batch.  A change needs a new
        workspace and a new ``set_context``; both follow from dropping the workspace key here.  Refused on fp8, 9-channel and
        IP-Adapter handles and together with Token Merging, T-GATE, DeepCache and ControlNet residuals."""
        if isinstance(layer_mask, bool) or not isinstance(layer_mask, int) or layer_mask < 0 or \
                layer_mask >> len(self.pag_block_names(self.config)):
            raise ValueError(f"layer_mask={layer_mask!r}: a PAG layer mask has one bit per transformer block "
                             f"({len(self.pag_block_names(self.config))} here; 0 = off)")
        if layer_mask:
            self._check_option(options.PAG)
        _lib.check(self._lib.sd_unet_set_pag(self._handle, layer_mask), "sd_unet_set_pag")
        if layer_mask != self._pag:
            self._pag = layer_mask
            self._ws_key = None
            self._tgate_ws.clear()

    # -- SAG (include/sd_hip.h::sd_unet_set_sag) --------------------------------------------------------
    @staticmethod
    def check_sag_handle(config, weight_dtype="bf16"):
        """What ``set_sag`` refuses about the handle, by name, without touching the GPU."""
        options.check(options.SAG, options.handle_options(config, weight_dtype))

    @staticmethod
    def sag_mid_grid(config, h: int, w: int):
        """(mh, mw) of the mid block's token grid under an ``h`` x ``w`` latent; SAG serves 4 .. 16 per side with the factor
        exactly 8 (``ValueError`` otherwise, by name)."""
        f = 2 ** (len(config.block_out_channels) - 1)
        mh, mw = h // f, w // f
        if f != 8 or h % 8 or w % 8 or not (4 <= mh <= 16 and 4 <= mw <= 16):
            raise ValueError(f"SAG: a {h}x{w} latent with {len(config.block_out_channels)} UNet levels gives a {mh}x{mw} mid grid at "
                             f"factor {f}; built for factor 8 and 4 .. 16 tokens per side (latents of 32 .. 128, multiples of 8)")
        return mh, mw

    def set_sag(self, on: bool, mass: Optional[torch.Tensor] = None) -> None:
        """Self-attention guidance: with ``on`` every forward also writes the attention mass of the mid block's self-attention,
        fp32 [unet_batch, mh * mw], into ``mass`` (a contiguous fp32 device tensor the caller keeps; the last one set is kept when
        None).  The forward's output does not change.  Off: the handle of before.  The prompt context sits at the same place in
        both kinds of plan, so toggling per forward keeps the workspace and its context.  Refused on fp8, 9-channel and IP-Adapter
        handles and together with PAG, Token Merging, T-GATE, DeepCache, ControlNet residuals and an image prompt."""
        if on:
            self._check_option(options.SAG)
            if mass is not None:
                if mass.dtype != torch.float32 or not mass.is_contiguous() or mass.device != self.device:
                    raise ValueError("set_sag: mass must be a contiguous fp32 tensor on the UNet's device")
                _lib.check(self._lib.sd_unet_set_sag_buffer(self._handle, mass.data_ptr(), mass.numel()), "sd_unet_set_sag_buffer")
                self._sag_mass = mass
            elif self._sag_mass is None:
                raise ValueError("set_sag(True) needs a mass buffer the first time")
        _lib.check(self._lib.sd_unet_set_sag(self._handle, 1 if on else 0), "sd_unet_set_sag")
        self._sag = bool(on)

    def clear_sag(self) -> None:
        """Capture off, the mass buffer and the second workspace released."""
        self.set_sag(False)
        _lib.check(self._lib.sd_unet_set_sag_buffer(self._handle, None, 0), "sd_unet_set_sag_buffer")
        self._sag_mass = None
        self._sag_ws.clear()
        self._sag_ctx_key = None

    def set_sag_context(self, encoder_hidden_states: torch.Tensor, height: Optional[int] = None, width: Optional[int] = None) -> None:
        """The prompt context of the SAG forward (``forward_latents(..., sag_forward=True)``), once per call: its own workspace,
        so the two forwards of a step alternate without refolding either context."""
        h, w = self.latent_size(height, width)
        ehs = encoder_hidden_states.to(self.device, torch.float32).contiguous()
        ub = ehs.shape[0]
        if ehs.shape[1] != self.config.context_len or ehs.shape[2] != self.config.cross_attention_dim:
            raise ValueError(f"encoder_hidden_states must be [N,{self.config.context_len},{self.config.cross_attention_dim}], "
                             f"got {tuple(ehs.shape)}")
        was = self._sag
        if was:
            self.set_sag(False)             # (the SAG forward runs the plain plan)
        try:
            key = (ub, h, w)
            if not self._sag_ws.holds(key):
                self._sag_ws.reserve(self._workspace_bytes(ub, -1, h, w), key)
            _lib.check(self._lib.sd_unet_set_context_hw(self._handle, _lib.current_stream(), ehs.data_ptr(), ub, -1, h, w,
                                                        self._sag_ws.ptr, self._sag_ws.nbytes), "sd_unet_set_context_hw")
        finally:
            if was:
                self.set_sag(True)
        self._sag_ctx_key = (ub, h, w)

    # -- FreeU (include/sd_hip.h::sd_unet_set_freeu) -------------------------------------------------
    @staticmethod
    def check_freeu_args(s1, s2, b1, b2, weight_dtype="bf16"):
        """The arguments of ``set_freeu`` checked, by name, without touching the GPU; returns them as four floats."""
        out = []
        for name, v in (("s1", s1), ("s2", s2), ("b1", b1), ("b2", b2)):
            if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(float(v)) or not float(v) > 0.0 \
                    or float(v) > 3.0e38:
                raise ValueError(f"{name}={v!r}: every FreeU factor must be a finite number > 0 (diffusers switches FreeU off "
                                 "silently when a factor is 0; here that is an error: use disable_freeu())")
            out.append(float(v))
        options.check(options.FREEU, options.handle_options(None, weight_dtype))
        return tuple(out)

    def set_freeu(self, s1: float, s2: float, b1: float, b2: float) -> None:
        """diffusers ``enable_freeu``: in up blocks 0 and 1 every resnet reads the hidden tensor with its first half of the
        channels times ``b1`` / ``b2`` and the skip tensor with its four lowest Fourier modes times ``s1`` / ``s2``.  The
        factors are read at launch: changing them builds no plan.  Switching on needs a new workspace and a new
        ``set_context``; both follow from dropping the workspace key here."""
        f = self.check_freeu_args(s1, s2, b1, b2, self.weight_dtype)
        _lib.check(self._lib.sd_unet_set_freeu(self._handle, *f), "sd_unet_set_freeu")
        if self._freeu is None:
            self._ws_key = None
        self._freeu = f

    def disable_freeu(self) -> None:
        """Forwards are again those of a UNet that never saw FreeU, bit for bit."""
        _lib.check(self._lib.sd_unet_disable_freeu(self._handle), "sd_unet_disable_freeu")
        if self._freeu is not None:
            self._ws_key = None
        self._freeu = None

    # -- T-GATE (include/sd_hip.h::sd_unet_set_tgate_hw) -----------------------------------------------
    TGATE_OFF, TGATE_CAPTURE, TGATE_REUSE = 0, 1, 2

    @staticmethod
    def check_tgate_support(config, weight_dtype="bf16"):
        """What T-GATE refuses on the UNet's side, by name, without touching the GPU."""
        options.check(options.TGATE, options.handle_options(config, weight_dtype))

    def tgate_blocks(self, latent_batch: int, height: Optional[int] = None, width: Optional[int] = None):
        """The cache slices of ``latent_batch`` latents, one per transformer block in plan order (down, mid, up): dicts of
        ``offset`` (bytes into the cache buffer), ``rows`` (= latent_batch * tokens) and ``channels``."""
        lh, lw = self.latent_size(height, width)
        n = self._lib.sd_unet_tgate_block_info_hw(self._handle, -1, latent_batch, lh, lw, None, None, None)
        if n < 0:
            _lib.check(-1, "sd_unet_tgate_block_info_hw")
        out = []
        for i in range(n):
            off, rows, ch = C.c_longlong(), C.c_longlong(), C.c_int()
            if self._lib.sd_unet_tgate_block_info_hw(self._handle, i, latent_batch, lh, lw, C.byref(off), C.byref(rows), C.byref(ch)) < 0:
                _lib.check(-1, "sd_unet_tgate_block_info_hw")
            out.append(dict(offset=off.value, rows=rows.value, channels=ch.value))
        return out

    def _reserve_tgate_cache(self, latent_batch: int, h: int, w: int) -> Workspace:
        n = Workspace.bytes_or_raise(self._lib.sd_unet_tgate_bytes_hw(self._handle, latent_batch, h, w), "sd_unet_tgate_bytes_hw")
        self._tgate_cache.reserve(n)        # (grow-only: kept and reused while it fits)
        return self._tgate_cache

    def tgate_cache(self, latent_batch: int, height: Optional[int] = None, width: Optional[int] = None) -> torch.Tensor:
        """The cache buffer for ``latent_batch`` latents at this size (uint8, with slack to align it; kept while it fits)."""
        return self._reserve_tgate_cache(latent_batch, *self.latent_size(height, width)).tensor

    def tgate_cache_block(self, block: int, latent_batch: int, height: Optional[int] = None, width: Optional[int] = None) -> torch.Tensor:
        """Slice ``block`` of the cache as a bf16 tensor [rows, channels] (a view of the buffer)."""
        info = self.tgate_blocks(latent_batch, height, width)[block]
        buf, off = self._tgate_cache.view, info["offset"]
        return buf[off:off + info["rows"] * info["channels"] * 2].view(torch.bfloat16).view(info["rows"], info["channels"])

    def _tgate_capture_bytes(self, unet_batch: int, latent_batch: int, h: int, w: int) -> int:
        """Workspace bytes of the capture plans of ``unet_batch`` (the handle is left off)."""
        buf = self._reserve_tgate_cache(latent_batch, h, w)
        _lib.check(self._lib.sd_unet_set_tgate_hw(self._handle, self.TGATE_CAPTURE, buf.ptr, buf.nbytes, latent_batch, h, w),
                   "sd_unet_set_tgate_hw")
        try:
            return self._workspace_bytes(unet_batch, self.cache_branch_id, h, w)
        finally:
            _lib.check(self._lib.sd_unet_set_tgate_hw(self._handle, self.TGATE_OFF, None, 0, 0, 0, 0), "sd_unet_set_tgate_hw")

    def reserve_tgate(self, latent_batch: Optional[int], height: Optional[int] = None, width: Optional[int] = None) -> None:
        """Before ``set_context``: size the next workspace for the capture plans of ``latent_batch`` latents at this size as well,
        so that ``set_tgate(TGATE_CAPTURE, ...)`` in the middle of a run keeps the workspace and the prompt context in it.
        ``None``: the workspaces are again those of a UNet that never saw T-GATE."""
        new = None if latent_batch is None else (int(latent_batch), *self.latent_size(height, width))
        if new != self._tgate_reserve:
            self._tgate_reserve = new
            self._ws_key = None
            if new is None:
                self._tgate_ws.clear()
                self._tgate_cache.clear()

    def set_tgate(self, mode: int, latent_batch: int = 0, height: Optional[int] = None, width: Optional[int] = None) -> None:
        """T-GATE state of the handle.  ``TGATE_CAPTURE``: the next forward (UNet batch ``latent_batch``, or twice it for a CFG
        pair) also fills the cache: per transformer block the mean of the pair's cross-attention outputs.  ``TGATE_REUSE``:
        forwards run at UNet batch ``latent_batch`` on the latents alone, with the cached tensor in place of norm2 and attn2;
        they need no ``set_context``.  ``TGATE_OFF``: forwards are again those of a UNet that never saw it, bit for bit."""
        if mode == self.TGATE_OFF:
            _lib.check(self._lib.sd_unet_set_tgate_hw(self._handle, 0, None, 0, 0, 0, 0), "sd_unet_set_tgate_hw")
            self._tgate = None
            self._grow_workspace_for_control()      # (a workspace sized while capturing: the plain plans must fit it too)
            return
        self._check_option(options.TGATE)
        h, w = self.latent_size(height, width)
        buf = self._reserve_tgate_cache(latent_batch, h, w)
        _lib.check(self._lib.sd_unet_set_tgate_hw(self._handle, int(mode), buf.ptr, buf.nbytes, int(latent_batch), h, w),
                   "sd_unet_set_tgate_hw")
        self._tgate = (int(mode), int(latent_batch), h, w)
        if mode == self.TGATE_CAPTURE and self._ws is not None and self._ws_key is not None and self._ws_key[2:] == (h, w):
            self._grow_workspace_for_control()      # (a workspace sized before the capture plans were asked for: keep its context)

    def _tgate_workspace(self, unet_batch: int, h: int, w: int) -> Workspace:
        key = (unet_batch, h, w)
        if not self._tgate_ws.holds(key):
            self._tgate_ws.reserve(self._workspace_bytes(unet_batch, -1, h, w), key)
        return self._tgate_ws

    def plan_count(self) -> int:
        """Execution plans the handle has built so far."""
        return int(self._lib.sd_unet_plan_count(self._handle))

    # -- forward ---------------------------------------------------------------------------
    def forward_latents(self, latents: torch.Tensor, unet_batch: int, timestep: float,
                        out: Optional[torch.Tensor] = None, cache_mode: int = CACHE_OFF, sag_forward: bool = False) -> torch.Tensor:
        """eps [unet_batch,4,H,W] fp32 for fp32 NCHW ``latents`` [B,4,H,W]; ``unet_batch`` is B or
        a multiple of it (CFG: 2B, the duplication is fused).  H and W are taken from ``latents``: each a
        multiple of 2^(levels - 1).  ``set_context`` must have run for this batch and size.  ``sag_forward``: the second
        forward of a SAG step -- the workspace and context of ``set_sag_context``, capture off."""
        if latents.dim() != 4 or latents.shape[1] != LATENT_CHANNELS:
            raise ValueError(f"latents must be [B,{LATENT_CHANNELS},H,W], got {tuple(latents.shape)}")
        b, c, h, w = latents.shape
        if self.config.in_channels == 9 and (self._inpaint_key is None or self._inpaint_key[1:] != (h, w)
                                             or unet_batch % self._inpaint_key[0]):
            raise _lib.SdHipError(f"this UNet has in_channels = 9: set_inpaint_cond(mask, masked_latents) must be called for "
                                  f"this batch and size ({h}x{w}) first")
        gated = self._tgate is not None and self._tgate[0] == self.TGATE_REUSE      # (no prompt context behind the gate)
        if sag_forward:
            if self._sag or gated or cache_mode != CACHE_OFF:
                raise _lib.SdHipError("a SAG forward runs with capture off (set_sag(False)), without T-GATE and DeepCache")
            if self._sag_ctx_key != (unet_batch, h, w):
                raise _lib.SdHipError(f"set_sag_context(encoder_hidden_states, {h}, {w}) must be called for this batch and size first")
        elif not gated and (self._ctx_key is None or self._ctx_key[2:] != (unet_batch, h, w)):
            raise _lib.SdHipError(f"set_context(encoder_hidden_states, {h}, {w}) must be called for this batch and size first")
        if self._ip_on and (unet_batch, self.cache_branch_id, h, w) not in self._ip_keys:
            raise _lib.SdHipError(f"this UNet runs with an IP-Adapter image prompt: set_ip_adapter(image_embeds, scale, {h}, {w}) must "
                                  f"be called for this batch ({unet_batch}) and size after set_context (or clear_ip_adapter())")
        if self._control is not None and self._control[2:] != (unet_batch, h, w):
            raise _lib.SdHipError(f"the ControlNet residuals were set for batch {self._control[2]} at {self._control[3]}x{self._control[4]}: "
                                  f"set_control_residuals for this batch ({unet_batch}) and size ({h}x{w}), or clear_control_residuals()")
        if latents.dtype != torch.float32 or not latents.is_contiguous() or latents.device != self.device:
            latents = latents.to(self.device, torch.float32).contiguous()
        if out is None:
            out = torch.empty((unet_batch, self.config.out_channels, h, w), dtype=torch.float32, device=self.device)
        ws = self._sag_ws if sag_forward else self._tgate_workspace(unet_batch, h, w) if gated else self._reserve(unet_batch, h, w)
        _lib.check(self._lib.sd_unet_forward_hw(self._handle, _lib.current_stream(), latents.data_ptr(), b, unet_batch, h, w,
                                                float(timestep), out.data_ptr(), ws.ptr, ws.nbytes,
                                                cache_mode, self.cache_branch_id), "sd_unet_forward_hw")
        return out

    # -- fp8 activation-scale calibration (include/sd_hip.h::sd_unet_calibrate_fp8) ---------------------------------
    def calibrate_fp8(self, latents: torch.Tensor, unet_batch: int, timesteps, margin: float = 2.0) -> Dict[str, float]:
        """Per-tensor e4m3 activation scales from the amax observed on ``latents`` at each of ``timesteps`` (the context of
        ``set_context`` is used; ``unet_batch`` as for ``forward_latents``).  Returns ``fp8_scales()``.
        Calibration runs at the square ``sample_size`` latent; the per-tensor scales it sets are reused by the plans of
        every latent size (the same tensors, named after their modules)."""
        if self.weight_dtype != "fp8_e4m3":
            raise _lib.SdHipError("calibrate_fp8: the handle was not created with weight_dtype='fp8'")
        if self.cache_branch_id != -1:
            # sd_unet_calibrate_fp8 runs the plan WITHOUT DeepCache; a workspace sized and a context laid out for a cache
            # branch's plan would be read at another plan's offsets
            raise _lib.SdHipError("calibrate_fp8: call set_deepcache(-1) and set_context(...) first (the calibration pass runs "
                                  "the plan without DeepCache)")
        s = self.config.sample_size
        if self._ctx_key is None or self._ctx_key[2:] != (unet_batch, s, s):
            raise _lib.SdHipError("set_context(encoder_hidden_states) must be called for this batch first (at sample_size)")
        latents = latents.to(self.device, torch.float32).contiguous()
        if tuple(latents.shape[1:]) != (LATENT_CHANNELS, s, s):
            raise ValueError(f"calibrate_fp8: latents must be [B,{LATENT_CHANNELS},{s},{s}] (sample_size), got {tuple(latents.shape)}")
        ws = self._reserve(unet_batch)
        for t in timesteps:
            _lib.check(self._lib.sd_unet_calibrate_fp8(self._handle, _lib.current_stream(), latents.data_ptr(), latents.shape[0],
                                                       unet_batch, float(t), float(margin), ws.ptr, ws.nbytes),
                       "sd_unet_calibrate_fp8")
        return self.fp8_scales()

    def fp8_scales(self, with_amax: bool = False) -> Dict[str, float]:
        """{tensor name: scale} of every e4m3 activation tensor known so far (``with_amax``: (scale, observed amax))."""
        out = {}
        name = C.create_string_buffer(256)
        sc, am = C.c_float(), C.c_float()
        for i in range(self._lib.sd_unet_fp8_scale_count(self._handle)):
            _lib.check(self._lib.sd_unet_fp8_scale_info(self._handle, i, name, 256, C.byref(sc), C.byref(am)), "sd_unet_fp8_scale_info")
            out[name.value.decode()] = (sc.value, am.value) if with_amax else sc.value
        return out

    def set_fp8_scales(self, scales: Dict[str, float]) -> None:
        # the e4m3 activation tensors get their names when a plan is built: make sure one exists (batch 1, no DeepCache)
        if self._lib.sd_unet_workspace_bytes(self._handle, 1, -1) < 0:
            _lib.check(-1, "sd_unet_workspace_bytes")
        for k, v in scales.items():
            _lib.check(self._lib.sd_unet_set_fp8_scale(self._handle, k.encode(), float(v)), f"sd_unet_set_fp8_scale({k})")

    KIND_NAMES = {0: "sinusoid", 1: "gemv", 2: "conv_in", 3: "groupnorm", 4: "conv3x3", 5: "gemm", 6: "layernorm",
                  7: "attention", 8: "conv_out", 9: "hypertile_gather", 10: "hypertile_scatter", 11: "pag_identity", 12: "sag_mass", 16: "conv3x3_fp8", 17: "gemm_fp8", 18: "xattn_fused",
                  19: "replicate", 20: "conv3x3_gemm", 21: "conv3x3_halo_subpix", 22: "ip_xattn", 23: "residual_add",
                  24: "tgate_capture", 25: "tgate_apply", 26: "tgate_zero",
                  27: "tome_match", 28: "tome_select", 29: "tome_merge", 30: "tome_unmerge", 31: "freeu"}

    def forward_profiled(self, latents: torch.Tensor, unet_batch: int, timestep: float, cache_mode: int = CACHE_OFF):
        """One forward with a hipEvent pair around every launch (measurement only, synchronises).
        Returns {kind: dict(ms, launches, flops, bytes)}.  Square ``sample_size`` latents only."""
        latents = latents.to(self.device, torch.float32).contiguous()
        s = self.config.sample_size
        if tuple(latents.shape[2:]) != (s, s):
            raise ValueError(f"forward_profiled: {s}x{s} latents only, got {tuple(latents.shape)}")
        out = torch.empty((unet_batch, self.config.out_channels, latents.shape[2], latents.shape[3]),
                          dtype=torch.float32, device=self.device)
        gated = self._tgate is not None and self._tgate[0] == self.TGATE_REUSE
        ws = self._tgate_workspace(unet_batch, s, s) if gated else self._reserve(unet_batch)
        ms, fl, by = (C.c_double * 32)(), (C.c_double * 32)(), (C.c_double * 32)()
        ln = (C.c_longlong * 32)()
        _lib.check(self._lib.sd_unet_forward_profiled(
            self._handle, _lib.current_stream(), latents.data_ptr(), latents.shape[0], unet_batch, float(timestep),
            out.data_ptr(), ws.ptr, ws.nbytes, cache_mode, self.cache_branch_id, ms, ln, fl, by),
            "sd_unet_forward_profiled")
        return {n: dict(ms=ms[i], launches=ln[i], flops=fl[i], bytes=by[i]) for i, n in self.KIND_NAMES.items()
                if ln[i] or i < 9}

    def __call__(self, sample: torch.Tensor, timestep, encoder_hidden_states: torch.Tensor = None,
                 timestep_cond=None, cross_attention_kwargs=None, added_cond_kwargs=None, return_dict: bool = False,
                 down_block_additional_residuals=None, mid_block_additional_residual=None, **kwargs):
        """diffusers-style call of the reference loop (``src/models.py:227-235``).  ``timestep_cond`` ([B, d] or [d]) is
        the guidance embedding of an LCM-distilled UNet: one row for the whole batch (ONE_ROW_RULE); None runs without it.
        ``down_block_additional_residuals`` (twelve NCHW float tensors, already scaled) and
        ``mid_block_additional_residual``: a ControlNet's outputs as diffusers passes them; they are converted to the
        residual buffer (one bf16 rounding), added at scale 1 for this call and cleared after it.  Without them the call
        leaves the handle as it is: residuals set through ``set_control_residuals`` stay in force until
        ``clear_control_residuals``."""
        if (down_block_additional_residuals is None) != (mid_block_additional_residual is None):
            raise NotImplementedError("down_block_additional_residuals and mid_block_additional_residual go together (a ControlNet's "
                                      "outputs; a T2I-Adapter's down residuals alone are not built)")
        emb = None
        if added_cond_kwargs is not None:
            if self.config.ip_adapter_embed_dim is None:
                raise NotImplementedError("added_cond_kwargs is not part of the SD-1.5 hot path (this UNet has no IP-Adapter)")
            if set(added_cond_kwargs) != {"image_embeds"}:
                raise NotImplementedError(f"added_cond_kwargs {sorted(added_cond_kwargs)}: only {{'image_embeds': ...}} of one "
                                          "IP-Adapter is built")
            emb = self._call_image_embeds(added_cond_kwargs["image_embeds"], sample.shape[0])
        self._apply_timestep_cond(timestep_cond)
        h, w = sample.shape[2], sample.shape[3]
        key = (encoder_hidden_states.data_ptr(), encoder_hidden_states._version, sample.shape[0], h, w)
        if self._ctx_key != key:
            self.set_context(encoder_hidden_states, h, w)
        if emb is None:
            if self._ip_on:
                self.clear_ip_adapter()
        else:
            ip_call = (emb.data_ptr(), emb._version, float(self.ip_adapter_scale), sample.shape[0], self.cache_branch_id, h, w)
            if self._ip_call != ip_call or ip_call[3:] not in self._ip_keys:
                self.set_ip_adapter(emb, self.ip_adapter_scale, h, w)
                self._ip_call = ip_call
        t = float(timestep.item()) if torch.is_tensor(timestep) else float(timestep)
        if down_block_additional_residuals is not None:
            from .controlnet import pack_residuals
            buf = pack_residuals(down_block_additional_residuals, mid_block_additional_residual, self.config, self.device)
            self.set_control_residuals(buf, 1.0, sample.shape[0], h, w)
            try:
                eps = self.forward_latents(sample, sample.shape[0], t)
            finally:
                self.clear_control_residuals()
        else:
            eps = self.forward_latents(sample, sample.shape[0], t)      # (residuals set with set_control_residuals stay in force)
        return (eps.to(sample.dtype),)

    def _call_image_embeds(self, image_embeds, batch: int) -> torch.Tensor:
        """``added_cond_kwargs["image_embeds"]`` of diffusers: a tensor or a one-element list, [N, E] or [N, 1, E]."""
        if isinstance(image_embeds, (list, tuple)):
            if len(image_embeds) != 1:
                raise NotImplementedError(f"image_embeds: a list of {len(image_embeds)} (several IP-Adapters at once are not built)")
            image_embeds = image_embeds[0]
        e = self.config.ip_adapter_embed_dim
        if not torch.is_tensor(image_embeds):
            raise ValueError("image_embeds must be a tensor or a one-element list of tensors")
        if image_embeds.dim() == 3:
            if image_embeds.shape[1] != 1:
                raise NotImplementedError(f"image_embeds {tuple(image_embeds.shape)}: several images per sample are not built")
            image_embeds = image_embeds[:, 0]
        if image_embeds.dim() != 2 or image_embeds.shape[1] != e or image_embeds.shape[0] != batch:
            raise ValueError(f"image_embeds must be [{batch}, {e}] or [{batch}, 1, {e}], got {tuple(image_embeds.shape)}")
        return image_embeds

    ONE_ROW_RULE = "timestep_cond must be one row for the whole batch (one guidance scale per call)"

    def _apply_timestep_cond(self, timestep_cond) -> None:
        if timestep_cond is None:
            if self._cond is not None:
                self.set_timestep_cond(None)
            return
        if self.config.time_cond_proj_dim is None:
            raise ValueError("timestep_cond given, but this UNet has no time_embedding.cond_proj (time_cond_proj_dim is None)")
        tc = torch.as_tensor(timestep_cond).detach().to(self.device, torch.float32)
        if tc.dim() == 2:
            if tc.shape[0] > 1 and not bool((tc == tc[:1]).all()):
                raise ValueError(f"{self.ONE_ROW_RULE}; got {tc.shape[0]} different rows")
            tc = tc[0]
        elif tc.dim() != 1:
            raise ValueError(f"timestep_cond must be [B, d] or [d], got {tuple(tc.shape)}")
        if self._cond is None or self._cond.shape != tc.shape or not torch.equal(self._cond, tc):
            self.set_timestep_cond(tc)

    def debug_tensor(self, name: str, unet_batch: int, numel: int, height: Optional[int] = None,
                     width: Optional[int] = None) -> torch.Tensor:
        """Tap ``name`` of the last forward; ``height`` / ``width``: its latent size (default ``sample_size``)."""
        out = torch.empty(numel, dtype=torch.float32)
        ws = self._reserve(unet_batch, height, width)
        _lib.check(self._lib.sd_unet_debug_tensor(self._handle, _lib.current_stream(), name.encode(), out.data_ptr(),
                                                  numel, ws.ptr, unet_batch, self.cache_branch_id),
                   "sd_unet_debug_tensor")
        return out
