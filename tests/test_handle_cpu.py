"""handle.py without a GPU and without the library: the aligned workspace and its two cache policies, the one parameter
loop, and the one ``__del__``."""
import ctypes

import pytest
import torch

from sonicdiffusionbayeslab_amd import _lib
from sonicdiffusionbayeslab_amd.handle import ALIGN, HipHandle, Workspace, load_params


class StubLib:
    """Records what the parameter loop and ``__del__`` hand the library."""

    def __init__(self, destroy_raises=False):
        self.loaded, self.destroyed, self.destroy_raises = [], [], destroy_raises

    def sd_unet_load_param(self, handle, name, ptr, numel):
        self.loaded.append((handle, name, ptr, numel))
        return 0

    def _destroy(self, which, handle):
        self.destroyed.append((which, handle))
        if self.destroy_raises:
            raise RuntimeError("destroy failed")

    def sd_unet_destroy(self, handle):
        self._destroy("sd_unet_destroy", handle)

    def sd_inception_destroy(self, handle):
        self._destroy("sd_inception_destroy", handle)

    def sd_last_error(self):
        return b"stub error"


# ------------------------------------------------------------------------------------------ Workspace
@pytest.mark.parametrize("n", [0, 1, 255, 256, 257])
def test_workspace_is_aligned_and_inside_its_buffer(n):
    assert ALIGN == 256                 # the slack check_workspace (csrc/unet.hip) is written for
    ws = Workspace("cpu")
    assert ws.tensor is None and ws.nbytes == 0
    assert ws.reserve(n) is True
    t = ws.tensor
    assert t.dtype == torch.uint8 and t.dim() == 1
    assert ws.nbytes == n and ws.ptr % 256 == 0
    assert ws.ptr >= t.data_ptr() and ws.ptr + ws.nbytes <= t.data_ptr() + t.numel()
    v = ws.view
    assert v.numel() == n and (n == 0 or v.data_ptr() == ws.ptr)
    ws.clear()
    assert ws.tensor is None and ws.key is None and ws.nbytes == 0


def test_exact_policy_follows_the_key_not_the_size():
    ws = Workspace("cpu")
    assert not ws.holds("a")
    assert ws.reserve(1000, key="a") is True
    first = ws.tensor
    assert ws.holds("a") and not ws.holds("b")
    assert ws.reserve(1000, key="a") is False and ws.tensor is first
    assert ws.reserve(5000, key="a") is False and ws.tensor is first         # the key says what the buffer was sized for
    assert ws.reserve(10, key="b") is True                                   # a new key: a new buffer, even a smaller one
    assert ws.tensor is not first and ws.nbytes == 10 and ws.key == "b"
    ws.key = None                                                            # what the UNet does to invalidate its workspace
    assert ws.tensor is not None and not ws.holds("b")
    assert ws.reserve(10, key="b") is True


def test_grow_only_policy_follows_the_size():
    ws = Workspace("cpu")
    assert ws.reserve(1000) is True
    first = ws.tensor
    assert ws.reserve(1000) is False and ws.reserve(10) is False and ws.reserve(0) is False
    assert ws.tensor is first and ws.nbytes == 1000
    assert ws.reserve(1001) is True
    assert ws.tensor is not first and ws.nbytes == 1001


def test_bytes_or_raise(monkeypatch):
    monkeypatch.setattr(_lib, "load", lambda: StubLib())
    assert Workspace.bytes_or_raise(0, "x_bytes") == 0 and Workspace.bytes_or_raise(12345, "x_bytes") == 12345
    with pytest.raises(_lib.SdHipError, match="x_bytes failed.*stub error"):
        Workspace.bytes_or_raise(-1, "x_bytes")


# ------------------------------------------------------------------------------------------ load_params
SHAPES = [("a.weight", (4, 3)), ("a.bias", (4,)), ("attn.to_q.weight", (6, 6))]


def state_dict(dtype=torch.float32):
    g = torch.Generator().manual_seed(3)
    return {n: torch.randn(s, generator=g).to(dtype) for n, s in SHAPES}


def test_load_params_names_the_missing_parameter():
    sd = state_dict()
    del sd["a.bias"]
    lib = StubLib()
    with pytest.raises(KeyError, match="state_dict lacks VAE parameter 'a.bias'"):
        load_params(lib, 7, SHAPES, sd, "VAE")
    assert [name for _, name, _, _ in lib.loaded] == [b"a.weight"]           # in order, up to the missing one


def test_load_params_gives_both_shapes():
    sd = state_dict()
    sd["a.weight"] = torch.zeros(3, 4)
    with pytest.raises(ValueError, match=r"a\.weight: expected shape \(4, 3\), got \(3, 4\)"):
        load_params(StubLib(), 7, SHAPES, sd, "UNet")


def test_load_params_hands_over_fp32_of_the_right_size():
    sd = state_dict(torch.float16)
    seen = {}

    class Reading(StubLib):
        def sd_unet_load_param(self, handle, name, ptr, numel):
            seen[name.decode()] = torch.tensor((ctypes.c_float * numel).from_address(ptr)[:])      # read as fp32, now
            return super().sd_unet_load_param(handle, name, ptr, numel)

    lib = Reading()
    load_params(lib, 7, SHAPES, sd, "CLIP")
    assert [(h, n, k) for h, n, _, k in lib.loaded] == [(7, b"a.weight", 12), (7, b"a.bias", 4), (7, b"attn.to_q.weight", 36)]
    for name, _ in SHAPES:
        assert torch.equal(seen[name], sd[name].float().reshape(-1))         # fp16 -> fp32 is exact


def test_load_params_reshapes_legacy_weights_only_when_asked():
    sd = state_dict()
    sd["attn.to_q.weight"] = sd["attn.to_q.weight"].reshape(6, 6, 1, 1)     # an attention weight stored as a 1x1 conv
    with pytest.raises(ValueError, match=r"attn\.to_q\.weight: expected shape \(6, 6\), got \(6, 6, 1, 1\)"):
        load_params(StubLib(), 7, SHAPES, sd, "VAE")
    lib = StubLib()
    load_params(lib, 7, SHAPES, sd, "VAE", reshape_legacy=True)
    assert lib.loaded[-1][1] == b"attn.to_q.weight" and lib.loaded[-1][3] == 36
    sd["a.bias"] = sd["a.bias"].reshape(4, 1, 1, 1)                          # only 4-D tensors for a 2-D shape are reshaped
    with pytest.raises(ValueError, match=r"a\.bias: expected shape \(4,\)"):
        load_params(StubLib(), 7, SHAPES, sd, "VAE", reshape_legacy=True)


def test_load_params_surfaces_the_library_error(monkeypatch):
    class Refusing(StubLib):
        def sd_unet_load_param(self, handle, name, ptr, numel):
            return -1

    lib = Refusing()
    monkeypatch.setattr(_lib, "load", lambda: lib)
    with pytest.raises(_lib.SdHipError, match=r"sd_unet_load_param\(a\.weight\) failed.*stub error"):
        load_params(lib, 7, SHAPES, state_dict(), "UNet")


# ------------------------------------------------------------------------------------------ HipHandle.__del__
class Inception(HipHandle):
    _destroy = "sd_inception_destroy"


def half_built(cls, lib=None, handle=None):
    obj = object.__new__(cls)           # as after an __init__ that raised part-way: only what was set so far
    if lib is not None:
        obj._lib = lib
    if handle is not None:
        obj._handle = handle
    return obj


@pytest.mark.parametrize("cls, symbol", [(HipHandle, "sd_unet_destroy"), (Inception, "sd_inception_destroy")])
def test_del_calls_the_destroy_symbol_of_the_class_once(cls, symbol):
    lib = StubLib()
    obj = half_built(cls, lib, 41)
    obj.__del__()
    assert lib.destroyed == [(symbol, 41)] and obj._handle is None
    obj.__del__()                                                            # a second call (interpreter teardown) is a no-op
    del obj
    assert lib.destroyed == [(symbol, 41)]


def test_del_tolerates_a_half_built_object_and_a_failing_destroy():
    half_built(HipHandle).__del__()                                          # neither _lib nor _handle
    lib = StubLib()
    half_built(HipHandle, lib).__del__()                                     # no _handle
    half_built(HipHandle, lib, 0).__del__()                                  # a handle that was never created
    assert lib.destroyed == []
    lib = StubLib(destroy_raises=True)
    obj = half_built(HipHandle, lib, 41)
    obj.__del__()                                                            # swallowed: __del__ must not raise
    assert lib.destroyed == [("sd_unet_destroy", 41)]
    obj._handle = None                                                       # (nothing to destroy when obj goes)


def test_the_old_workspace_names_sit_over_the_workspace():
    obj = half_built(HipHandle)
    obj._wsp = Workspace("cpu")
    assert obj._ws is None and obj._ws_key is None
    obj._wsp.reserve(100, key=(1, 8, 8))
    assert obj._ws is obj._wsp.tensor and obj._ws_key == (1, 8, 8)
    assert obj._ws_ptr(obj._ws) == obj._wsp.ptr and obj._ws.numel() - 256 == obj._wsp.nbytes       # the pair tests pass the ABI
    obj._ws_key = None
    assert obj._ws is not None and not obj._wsp.holds((1, 8, 8))
    obj._ws = None                                                           # frees the buffer
    assert obj._wsp.tensor is None


def test_no_gpu_is_an_error_naming_the_class(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(_lib.SdHipError, match="Inception needs an MI355X"):
        Inception("cuda:0")
