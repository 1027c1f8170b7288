"""FID features on libsdhip: the FID Inception-v3 ("pt_inception-2015-12-05", what torchmetrics'
``FrechetInceptionDistance`` runs through torch-fidelity's ``FeatureExtractorInceptionV3``; reference
``src/metrics/metrics.py:98-112``) as a HIP network, the fp64 statistics on the device and the Frechet distance on the host.

``HipInceptionFeatures`` takes the checkpoint's state dict (``<module>.conv.weight`` and
``<module>.bn.{weight,bias,running_mean,running_var}``; ``fc.*`` and ``num_batches_tracked`` are ignored), folds every
BatchNorm (eps 1e-3, running statistics) into its conv in fp64 and hands the folded fp32 weights to the library.  There is
no host fallback: without the library the class raises.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Dict, List, Tuple

import torch

from . import _lib
from .handle import HipHandle, Workspace

TAPS = (64, 192, 768, 2048)
BN_EPS = 1e-3


def check_feature(feature) -> int:
    if isinstance(feature, bool) or not isinstance(feature, int) or feature not in TAPS:
        raise ValueError(f"fid feature {feature!r}: one of {', '.join(str(t) for t in TAPS)} "
                         "(the pooled taps of the FID Inception-v3)")
    return feature


def conv_table() -> List[Tuple[str, Tuple[int, int, int, int]]]:
    """``[(module name, (Cout, Cin, kh, kw))]`` of the 94 conv blocks in forward order, as the library declares them (host
    only: no GPU is touched)."""
    lib = _lib.load()
    h = C.c_void_p()
    _lib.check(lib.sd_inception_create(C.byref(h)), "sd_inception_create")
    try:
        out = []
        name = C.create_string_buffer(128)
        shape = (C.c_longlong * 4)()
        for i in range(lib.sd_inception_num_convs(h)):
            _lib.check(lib.sd_inception_conv_info(h, i, name, 128, shape), "sd_inception_conv_info")
            out.append((name.value.decode(), tuple(int(s) for s in shape)))
        return out
    finally:
        lib.sd_inception_destroy(h)


def fold_state_dict(sd: Dict[str, torch.Tensor]) -> Dict[str, Tuple[torch.Tensor, torch.Tensor]]:
    """``{module: (folded weight fp32 OIHW, folded bias fp32)}``; KeyError / ValueError naming the first missing or
    mis-shaped key.  Host only."""
    out = {}
    for name, shape in conv_table():
        keys = {"w": f"{name}.conv.weight", "g": f"{name}.bn.weight", "b": f"{name}.bn.bias",
                "m": f"{name}.bn.running_mean", "v": f"{name}.bn.running_var"}
        for k in keys.values():
            if k not in sd:
                raise KeyError(f"Inception checkpoint lacks {k}")
        t = {s: sd[k].detach().to("cpu", torch.float64) for s, k in keys.items()}
        if tuple(t["w"].shape) != shape:
            raise ValueError(f"{keys['w']}: expected shape {shape}, got {tuple(t['w'].shape)}")
        for s in "gbmv":
            if tuple(t[s].shape) != (shape[0],):
                raise ValueError(f"{keys[s]}: expected shape {(shape[0],)}, got {tuple(t[s].shape)}")
        scale = t["g"] / torch.sqrt(t["v"] + BN_EPS)
        w = (t["w"] * scale.view(-1, 1, 1, 1)).float().contiguous()
        b = (t["b"] - t["m"] * scale).float().contiguous()
        out[name] = (w, b)
    return out


class HipInceptionFeatures(HipHandle):
    """uint8 images ``[B,3,H,W]`` (any size) -> fp32 features ``[B, feature]`` on the GPU."""
    _destroy = "sd_inception_destroy"

    def __init__(self, folded: Dict[str, Tuple[torch.Tensor, torch.Tensor]], device=None):
        super().__init__(device, resolve=True)
        h = self._handle
        _lib.check(self._lib.sd_inception_create(C.byref(h)), "sd_inception_create")
        with torch.cuda.device(self.device):
            for name, (w, b) in folded.items():
                _lib.check(self._lib.sd_inception_load_conv(h, name.encode(), w.data_ptr(), w.numel(), b.data_ptr(), b.numel()),
                           f"sd_inception_load_conv({name})")
            _lib.check(self._lib.sd_inception_finalize(h), "sd_inception_finalize")

    @classmethod
    def from_state_dict(cls, sd: Dict[str, torch.Tensor], device=None) -> "HipInceptionFeatures":
        return cls(fold_state_dict(sd), device=device)            # key / shape errors before any GPU work

    @classmethod
    def from_file(cls, path: str, device=None) -> "HipInceptionFeatures":
        return cls.from_state_dict(load_state_dict(path), device=device)

    def features(self, images: torch.Tensor, feature: int = 2048) -> torch.Tensor:
        check_feature(feature)
        if images.dtype != torch.uint8 or images.dim() != 4 or images.shape[1] != 3:
            raise ValueError(f"images must be uint8 [B,3,H,W], got {images.dtype} {tuple(images.shape)}")
        with torch.cuda.device(self.device):
            x = images.to(self.device).contiguous()
            b, _, h, w = x.shape
            self._wsp.reserve(Workspace.bytes_or_raise(self._lib.sd_inception_workspace_bytes(self._handle, b, feature),
                                                       "sd_inception_workspace_bytes"))        # (grow-only)
            out = torch.empty((b, feature), dtype=torch.float32, device=self.device)
            _lib.check(self._lib.sd_inception_features(self._handle, _lib.current_stream(), x.data_ptr(), b, h, w, feature,
                                                       out.data_ptr(), self._wsp.ptr, self._wsp.nbytes), "sd_inception_features")
            return out

    __call__ = features


def load_state_dict(path: str) -> Dict[str, torch.Tensor]:
    """A local ``.pth`` / ``.pt`` (``torch.load(weights_only=True)``) or ``.safetensors`` checkpoint."""
    if not os.path.isfile(str(path)):
        raise FileNotFoundError(f"Inception checkpoint {path!r} is not a local file")
    if str(path).endswith(".safetensors"):
        from safetensors.torch import load_file
        return dict(load_file(str(path)))
    sd = torch.load(str(path), map_location="cpu", weights_only=True)
    if isinstance(sd, dict) and "state_dict" in sd and isinstance(sd["state_dict"], dict):
        sd = sd["state_dict"]
    return sd


def fid_accumulate(features: torch.Tensor, total: torch.Tensor, cov_sum: torch.Tensor, count: torch.Tensor) -> None:
    """``total[D] += sum_b f``, ``cov_sum[D,D] += f^T f``, ``count += B`` in fp64 / int64 on the features' device, one launch
    (``sd_fid_accumulate``): the state torchmetrics keeps from ``features.double()``."""
    f = features.float().contiguous()
    b, d = f.shape
    assert total.dtype == torch.float64 and cov_sum.dtype == torch.float64 and count.dtype == torch.int64
    assert tuple(total.shape) == (d,) and tuple(cov_sum.shape) == (d, d) and count.numel() == 1
    assert total.is_contiguous() and cov_sum.is_contiguous() and total.device == f.device == cov_sum.device == count.device
    with torch.cuda.device(f.device):
        _lib.check(_lib.load().sd_fid_accumulate(_lib.current_stream(), f.data_ptr(), b, d, total.data_ptr(), cov_sum.data_ptr(),
                                                 count.data_ptr()), "sd_fid_accumulate")


def frechet_distance(mu1: torch.Tensor, sigma1: torch.Tensor, mu2: torch.Tensor, sigma2: torch.Tensor) -> torch.Tensor:
    """``|mu1 - mu2|^2 + tr S1 + tr S2 - 2 sum sqrt(eigvals(S1 S2)).real`` on the host in fp64 (torchmetrics'
    ``_compute_fid``); once per sweep point."""
    mu1, sigma1, mu2, sigma2 = (t.detach().to("cpu", torch.float64) for t in (mu1, sigma1, mu2, sigma2))
    a = (mu1 - mu2).square().sum(dim=-1)
    b = sigma1.trace() + sigma2.trace()
    c = torch.linalg.eigvals(sigma1 @ sigma2).sqrt().real.sum(dim=-1)
    return a + b - 2 * c


def make_synthetic_inception_state_dict(seed: int = 0) -> Dict[str, torch.Tensor]:
    """Seeded stand-in weights with the checkpoint's keys and shapes (He-scaled convs, BatchNorm near identity): for speed
    measurements and smoke runs where no checkpoint exists."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for name, (cout, cin, kh, kw) in conv_table():
        sd[f"{name}.conv.weight"] = torch.randn(cout, cin, kh, kw, generator=g) * (2.0 / (cin * kh * kw)) ** 0.5
        sd[f"{name}.bn.weight"] = 0.8 + 0.4 * torch.rand(cout, generator=g)
        sd[f"{name}.bn.bias"] = 0.1 * torch.randn(cout, generator=g)
        sd[f"{name}.bn.running_mean"] = 0.1 * torch.randn(cout, generator=g)
        sd[f"{name}.bn.running_var"] = 0.7 + 0.6 * torch.rand(cout, generator=g)
    return sd
