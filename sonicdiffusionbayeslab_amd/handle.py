"""What every wrapper of a libsdhip handle shares: the handle's lifetime, the one parameter loop and the aligned workspace.

The workspace contract with ``check_workspace`` (csrc/unet.hip): the library takes a pointer aligned to ``ALIGN`` bytes and
the bytes usable behind it.  ``Workspace`` allocates ``nbytes + ALIGN`` and hands out ``ptr`` / ``nbytes`` as a pair; passing
the raw buffer's ``numel()`` as the size would let a kernel write past the allocation.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import torch

from . import _lib

ALIGN = 256


def aligned(address: int) -> int:
    return (address + ALIGN - 1) // ALIGN * ALIGN


def resolve_device(device=None) -> torch.device:
    """``device`` as a torch.device; ``None``: the process's current CUDA device."""
    if device is None:
        return torch.device("cuda", torch.cuda.current_device())
    d = torch.device(device)
    return torch.device("cuda", torch.cuda.current_device()) if d.type == "cuda" and d.index is None else d


def load_params(lib, handle, shapes, state_dict, what: str, reshape_legacy: bool = False) -> None:
    """Every parameter ``shapes`` names ([(name, shape)]), checked for presence and shape, into the handle
    (``sd_unet_load_param`` copies; host-only, runs without a GPU).  Tensors of any float dtype are accepted -- diffusers
    checkpoints are fp16 on disk.  ``what``: the model's name in the KeyError.  ``reshape_legacy``: 4-D tensors where the
    shape is 2-D are reshaped (old VAE checkpoints store the attention weights as 1x1 convs).  Finalize is the caller's."""
    for name, shape in shapes:
        if name not in state_dict:
            raise KeyError(f"state_dict lacks {what} parameter {name!r}")
        t = state_dict[name].detach().to("cpu", torch.float32).contiguous()
        if reshape_legacy and t.dim() == 4 and len(shape) == 2:
            t = t.reshape(shape)
        if tuple(t.shape) != tuple(shape):
            raise ValueError(f"{name}: expected shape {shape}, got {tuple(t.shape)}")
        _lib.check(lib.sd_unet_load_param(handle, name.encode(), t.data_ptr(), t.numel()), f"sd_unet_load_param({name})")


class Workspace:
    """One uint8 device buffer with ``ALIGN`` bytes of slack: ``ptr`` is the aligned address inside ``tensor`` (the raw
    buffer), ``nbytes`` what is usable behind it.  Two cache policies, chosen per ``reserve``:

    * exact (a ``key``): a new buffer whenever the key differs, even for fewer bytes -- the UNet, the ControlNet, the VAE /
      TAESD halves and the CLIP text model, whose workspace holds state laid out for that key (the prompt context);
    * grow-only (no key): a new buffer only when this one is too small -- CLIP vision, ImageReward, Inception, the T-GATE
      cache."""

    def __init__(self, device):
        self.device = device
        self.clear()

    def clear(self) -> None:
        self.tensor: Optional[torch.Tensor] = None
        self.key = None
        self.ptr, self.nbytes = 0, 0

    def holds(self, key) -> bool:
        """Whether ``reserve(n, key)`` would keep the buffer (callers skip sizing the workspace then)."""
        return self.tensor is not None and self.key == key

    def reserve(self, nbytes: int, key=None) -> bool:
        """Returns whether it reallocated.  The old buffer is dropped BEFORE the new one is allocated: the two need not fit
        side by side."""
        if self.tensor is not None and (self.key == key if key is not None else self.nbytes >= nbytes):
            return False
        self.clear()
        self.tensor = torch.empty(nbytes + ALIGN, dtype=torch.uint8, device=self.device)
        self.ptr = aligned(self.tensor.data_ptr())
        self.nbytes, self.key = nbytes, key
        return True

    @property
    def view(self) -> torch.Tensor:
        """The usable bytes as an aligned slice of ``tensor``."""
        off = self.ptr - self.tensor.data_ptr()
        return self.tensor[off:off + self.nbytes]

    @staticmethod
    def bytes_or_raise(n: int, what: str) -> int:
        """``n`` of a ``*_workspace_bytes`` call, or the library's error for a negative one."""
        if n < 0:
            _lib.check(-1, what)
        return n


class HipHandle:
    """Base of every wrapper that owns one libsdhip handle: ``_lib``, ``_handle``, ``device``, the main workspace ``_wsp``
    and the one ``__del__``.

    Two device policies exist and each class keeps its own (the current device after building a model is behaviour):
    the UNet, the ControlNet and the VAE / TAESD halves call ``torch.cuda.set_device(self.device)`` once when built; the CLIP
    towers, ImageReward and Inception leave the current device alone and run every entry under
    ``with torch.cuda.device(self.device)``."""

    _destroy = "sd_unet_destroy"

    def __init__(self, device, resolve: bool = False):
        if not torch.cuda.is_available():
            raise _lib.SdHipError(f"{type(self).__name__} needs an MI355X (no CPU fallback exists)")
        self.device = resolve_device(device) if resolve else torch.device(device)
        self._lib = _lib.load()
        self._handle = C.c_void_p()
        self._wsp = Workspace(self.device)

    def __del__(self):
        try:
            if getattr(self, "_handle", None):
                getattr(self._lib, self._destroy)(self._handle)
                self._handle = None
        except Exception:
            pass

    def _finalize(self) -> None:
        _lib.check(self._lib.sd_unet_finalize(self._handle), "sd_unet_finalize")

    def _ws_ptr(self, ws: torch.Tensor) -> int:
        """The aligned address inside a raw workspace tensor (for callers that hold ``_workspace(...)``'s result)."""
        return aligned(ws.data_ptr())

    # the raw buffer and its key as attributes: ``obj._ws = None`` frees the buffer, ``obj._ws_key = None`` keeps it until the
    # next reserve with a key (what the UNet does when a setting changes the plans)
    @property
    def _ws(self) -> Optional[torch.Tensor]:
        return self._wsp.tensor

    @_ws.setter
    def _ws(self, value: None) -> None:
        assert value is None
        self._wsp.clear()

    @property
    def _ws_key(self):
        return self._wsp.key

    @_ws_key.setter
    def _ws_key(self, key) -> None:
        self._wsp.key = key
