"""CLIP score on libsdhip: the reference's quality metric (``quality_metrics.clip_score``, torchmetrics ``CLIPScore`` over
transformers ``CLIPModel``) with both towers on the GPU.

* ``HipClipVisionModel`` -- uint8 images ``[B,3,H,W]`` (any size) -> ``CLIPModel.get_image_features`` ``[B, projection_dim]``:
  ``CLIPImageProcessor`` (shortest edge -> ``image_size`` with Pillow's bicubic, bit-exact on the uint8 crop; centre crop;
  OpenAI mean / std), the ViT, ``post_layernorm`` of the class token and ``visual_projection``, all in libsdhip
  (``sd_clip_vision_create`` / ``sd_clip_vision_encode``).
* ``HipClipScorer`` -- a local ``CLIPModel`` directory (``config.json``, ``model.safetensors``, ``vocab.json`` /
  ``merges.txt``) -> per-pair ``100 cos(img, txt)`` (``sd_clip_score``); the text side is ``HipClipTextModel`` with the
  projection and ``ClipBpeTokenizer``.
"""
from __future__ import annotations

import ctypes as C
import json
import math
import os
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import torch

from . import _lib
from .clip import ClipBpeTokenizer, ClipTextConfig, HipClipTextModel
from .handle import HipHandle, Workspace, load_params, resolve_device

OPENAI_CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)
OPENAI_CLIP_STD = (0.26862954, 0.26130258, 0.27577711)
MAX_TOKENS = 320            # the ViT attention kernel's sequence limit (ViT-L/14 at 224: 257)


@dataclass
class ClipVisionConfig:
    hidden_size: int = 768
    num_hidden_layers: int = 12
    num_attention_heads: int = 12
    intermediate_size: int = 3072
    image_size: int = 224
    patch_size: int = 16
    projection_dim: int = 512
    layer_norm_eps: float = 1e-5
    hidden_act: str = "quick_gelu"      # or "gelu" (exact): the OpenCLIP ViT-H/14 image encoder of the IP-Adapters


HIDDEN_ACTS = {"quick_gelu": 0, "gelu": 1}      # include/sd_hip.h: SD_ACT_*


def clip_vision_param_shapes(cfg: ClipVisionConfig) -> List[Tuple[str, Tuple[int, ...]]]:
    """transformers ``CLIPVisionModelWithProjection`` / ``CLIPModel`` names of the vision tower, in module order."""
    H, I, P = cfg.hidden_size, cfg.intermediate_size, cfg.patch_size
    n_pos = (cfg.image_size // P) ** 2 + 1
    out: List[Tuple[str, Tuple[int, ...]]] = []
    add = lambda n, s: out.append((n, tuple(s)))
    add("vision_model.embeddings.class_embedding", (H,))
    add("vision_model.embeddings.patch_embedding.weight", (H, 3, P, P))
    add("vision_model.embeddings.position_embedding.weight", (n_pos, H))
    add("vision_model.pre_layrnorm.weight", (H,)); add("vision_model.pre_layrnorm.bias", (H,))
    for i in range(cfg.num_hidden_layers):
        p = f"vision_model.encoder.layers.{i}."
        for n in ("k_proj", "v_proj", "q_proj", "out_proj"):
            add(p + f"self_attn.{n}.weight", (H, H)); add(p + f"self_attn.{n}.bias", (H,))
        add(p + "layer_norm1.weight", (H,)); add(p + "layer_norm1.bias", (H,))
        add(p + "mlp.fc1.weight", (I, H)); add(p + "mlp.fc1.bias", (I,))
        add(p + "mlp.fc2.weight", (H, I)); add(p + "mlp.fc2.bias", (H,))
        add(p + "layer_norm2.weight", (H,)); add(p + "layer_norm2.bias", (H,))
    add("vision_model.post_layernorm.weight", (H,)); add("vision_model.post_layernorm.bias", (H,))
    add("visual_projection.weight", (cfg.projection_dim, H))
    return out


def make_synthetic_clip_vision_state_dict(cfg: ClipVisionConfig, seed: int = 555) -> Dict[str, torch.Tensor]:
    """Seeded vision-tower-shaped weights on the bf16 grid (for tests and benchmarks; no CLIP weights exist offline)."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for name, shape in clip_vision_param_shapes(cfg):
        if "embedding" in name:
            fan = shape[1] * shape[2] * shape[3] if name.endswith("patch_embedding.weight") else 0
            t = torch.randn(shape, generator=g) * (1.0 / math.sqrt(fan) if fan else 0.1)
        elif name.endswith(".bias"):
            t = torch.randn(shape, generator=g) * 0.02
        elif "norm" in name:
            t = 1.0 + 0.1 * torch.randn(shape, generator=g)
        else:
            t = torch.randn(shape, generator=g) / math.sqrt(shape[1])
        sd[name] = t.to(torch.bfloat16).float()
    return sd


def check_vision_config(cfg: ClipVisionConfig, hidden_act: Optional[str] = None, extended: bool = False) -> None:
    """The shapes libsdhip builds; ValueError naming the field otherwise (raised before any GPU work).  ``hidden_act``: the
    checkpoint's activation (default: the config's own).  ``extended``: also the tower of the IP-Adapters' image encoder --
    exact ``gelu`` and head dim 80 (ViT-H/14); without it the CLIP-score checkpoints' rule stands (``quick_gelu``, head dim
    64: the text tower beside it builds nothing else)."""
    hidden_act = cfg.hidden_act if hidden_act is None else hidden_act
    if hidden_act != "quick_gelu" and not (extended and hidden_act == "gelu"):
        raise ValueError(f"vision_config.hidden_act={hidden_act!r}: only 'quick_gelu' is built" +
                         (" (and 'gelu')" if extended else ""))
    H = cfg.hidden_size
    if H % 64 or H <= 0 or H > 1536:
        raise ValueError(f"vision_config.hidden_size={H}: a multiple of 64 up to 1536 is built")
    if cfg.intermediate_size % 64 or cfg.intermediate_size <= 0:
        raise ValueError(f"vision_config.intermediate_size={cfg.intermediate_size}: a multiple of 64 is built")
    if cfg.num_attention_heads <= 0 or H % cfg.num_attention_heads or H // cfg.num_attention_heads not in ((64, 80) if extended else (64,)):
        raise ValueError(f"vision_config.num_attention_heads={cfg.num_attention_heads}: head dim 64 is built" +
                         (" (and 80)" if extended else ""))
    if cfg.patch_size <= 0 or cfg.image_size % cfg.patch_size:
        raise ValueError(f"vision_config.patch_size={cfg.patch_size} must divide image_size={cfg.image_size}")
    if (cfg.image_size // cfg.patch_size) ** 2 + 1 > MAX_TOKENS:
        raise ValueError(f"vision_config.image_size={cfg.image_size}: {(cfg.image_size // cfg.patch_size) ** 2 + 1} tokens "
                         f"(at most {MAX_TOKENS} are built)")
    if cfg.projection_dim <= 0 or cfg.projection_dim % 4:
        raise ValueError(f"projection_dim={cfg.projection_dim}: a multiple of 4 is built")
    if abs(cfg.layer_norm_eps - 1e-5) > 1e-12:
        raise ValueError(f"vision_config.layer_norm_eps={cfg.layer_norm_eps}: 1e-5 is built")


def check_text_config(cfg: ClipTextConfig, hidden_act: str = "quick_gelu") -> None:
    if hidden_act != "quick_gelu":
        raise ValueError(f"text_config.hidden_act={hidden_act!r}: only 'quick_gelu' is built")
    H = cfg.hidden_size
    if H % 64 or H <= 0 or H > 1536:
        raise ValueError(f"text_config.hidden_size={H}: a multiple of 64 up to 1536 is built")
    if cfg.intermediate_size % 64 or cfg.intermediate_size <= 0:
        raise ValueError(f"text_config.intermediate_size={cfg.intermediate_size}: a multiple of 64 is built")
    if cfg.num_attention_heads <= 0 or H % cfg.num_attention_heads or H // cfg.num_attention_heads not in (16, 64):
        raise ValueError(f"text_config.num_attention_heads={cfg.num_attention_heads}: head dim 64 (or 16) is built")
    if not 1 <= cfg.max_position_embeddings <= 128:
        raise ValueError(f"text_config.max_position_embeddings={cfg.max_position_embeddings}: 1..128 are built")
    if abs(cfg.layer_norm_eps - 1e-5) > 1e-12:
        raise ValueError(f"text_config.layer_norm_eps={cfg.layer_norm_eps}: 1e-5 is built")


class HipClipVisionModel(HipHandle):
    """``CLIPModel.get_image_features(processor(images).pixel_values)`` on libsdhip: uint8 ``[B,3,H,W]`` -> fp32
    ``[B, projection_dim]``.  One plan (and workspace size) per (batch, H, W)."""

    def __init__(self, config: ClipVisionConfig, state_dict: Dict[str, torch.Tensor], device=None):
        """``device``: where the weights live and the tower runs (``None``: the current device); the process's current
        device is left as it is."""
        check_vision_config(config, extended=True)
        super().__init__(device, resolve=True)
        self.config = config
        self._sized = None                  # the (batch, H, W) the workspace was last sized for (grow-only: it may be larger)
        with torch.cuda.device(self.device):
            self._build(config, state_dict)

    def _build(self, config: ClipVisionConfig, state_dict: Dict[str, torch.Tensor]) -> None:
        c = _lib.SdClipVisionConfig(config.hidden_size, config.num_hidden_layers, config.num_attention_heads,
                                    config.intermediate_size, config.image_size, config.patch_size, config.projection_dim,
                                    config.layer_norm_eps, HIDDEN_ACTS[config.hidden_act])
        _lib.check(self._lib.sd_clip_vision_create(C.byref(c), C.byref(self._handle)), "sd_clip_vision_create")
        load_params(self._lib, self._handle, clip_vision_param_shapes(config), state_dict, "CLIP vision")
        self._finalize()

    def encode(self, images: torch.Tensor) -> torch.Tensor:
        with torch.cuda.device(self.device):
            return self._encode(images)

    def _encode(self, images: torch.Tensor) -> torch.Tensor:
        if images.dtype != torch.uint8 or images.dim() != 4 or images.shape[1] != 3:
            raise ValueError(f"images must be uint8 [B,3,H,W], got {images.dtype} {tuple(images.shape)}")
        x = images.to(self.device).contiguous()
        b, _, h, w = x.shape
        if self._sized != (b, h, w):
            self._wsp.reserve(Workspace.bytes_or_raise(self._lib.sd_clip_vision_workspace_bytes(self._handle, b, h, w),
                                                       "sd_clip_vision_workspace_bytes"))
            self._sized = (b, h, w)
        out = torch.empty((b, self.config.projection_dim), dtype=torch.float32, device=self.device)
        _lib.check(self._lib.sd_clip_vision_encode(self._handle, _lib.current_stream(), x.data_ptr(), b, h, w, out.data_ptr(),
                                                   self._wsp.ptr, self._wsp.nbytes), "sd_clip_vision_encode")
        return out

    __call__ = encode


def clip_score_pairs(image_embeds: torch.Tensor, text_embeds: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """``(raw, score)``: ``100 cos`` per pair and ``max(raw, 0)``, fp32 on the embeddings' device (``sd_clip_score``)."""
    with torch.cuda.device(image_embeds.device):
        return _clip_score_pairs(image_embeds, text_embeds)


def _clip_score_pairs(image_embeds: torch.Tensor, text_embeds: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    lib = _lib.load()
    a = image_embeds.float().contiguous()
    t = text_embeds.to(a.device, torch.float32).contiguous()
    if a.shape != t.shape or a.dim() != 2:
        raise ValueError(f"embeddings must both be [B, D], got {tuple(a.shape)} and {tuple(t.shape)}")
    raw = torch.empty(a.shape[0], dtype=torch.float32, device=a.device)
    score = torch.empty_like(raw)
    _lib.check(lib.sd_clip_score(_lib.current_stream(), a.data_ptr(), t.data_ptr(), a.shape[0], a.shape[1], raw.data_ptr(),
                                 score.data_ptr()), "sd_clip_score")
    return raw, score


def _read_json(path: str) -> dict:
    with open(path, encoding="utf-8") as f:
        return json.load(f)


def read_clip_configs(model_dir: str):
    """``(text_cfg, vision_cfg, eos_token_id or None for argmax pooling)`` from a local CLIPModel directory; ValueError
    naming the field for anything libsdhip does not build."""
    j = _read_json(os.path.join(model_dir, "config.json"))
    tj, vj = j.get("text_config", {}), j.get("vision_config", {})
    proj = int(j.get("projection_dim", 512))
    tk = ("vocab_size", "hidden_size", "num_hidden_layers", "num_attention_heads", "intermediate_size",
          "max_position_embeddings", "layer_norm_eps")
    tcfg = ClipTextConfig(**{k: tj[k] for k in tk if k in tj})
    vk = ("hidden_size", "num_hidden_layers", "num_attention_heads", "intermediate_size", "image_size", "patch_size",
          "layer_norm_eps")
    vcfg = ClipVisionConfig(projection_dim=proj, **{k: vj[k] for k in vk if k in vj})
    check_text_config(tcfg, tj.get("hidden_act", "quick_gelu"))
    check_vision_config(vcfg, vj.get("hidden_act", "quick_gelu"))
    pp = os.path.join(model_dir, "preprocessor_config.json")
    if os.path.isfile(pp):
        p = _read_json(pp)
        size = p.get("size", {})
        short = size.get("shortest_edge", size) if isinstance(size, dict) else size
        crop = p.get("crop_size", vcfg.image_size)
        crop = (crop.get("height"), crop.get("width")) if isinstance(crop, dict) else (crop, crop)
        checks = [("size", short == vcfg.image_size), ("crop_size", crop == (vcfg.image_size, vcfg.image_size)),
                  ("resample", p.get("resample", 3) == 3),
                  ("image_mean", all(abs(a - b) < 1e-7 for a, b in zip(p.get("image_mean", OPENAI_CLIP_MEAN), OPENAI_CLIP_MEAN))),
                  ("image_std", all(abs(a - b) < 1e-7 for a, b in zip(p.get("image_std", OPENAI_CLIP_STD), OPENAI_CLIP_STD))),
                  ("rescale_factor", abs(p.get("rescale_factor", 1 / 255) - 1 / 255) < 1e-12)]
        for flag in ("do_resize", "do_center_crop", "do_rescale", "do_normalize"):
            checks.append((flag, p.get(flag, True) is True))
        for name, ok in checks:
            if not ok:
                raise ValueError(f"preprocessor_config.{name}={p.get(name)!r}: only CLIP's default preprocessing is built")
    # transformers' CLIPTextTransformer pools at argmax(input_ids) when eos_token_id == 2 (the original openai configs),
    # otherwise at the first eos_token_id
    # (a text_config without the key gets transformers' CLIPTextConfig default, 49407: first-EOS pooling)
    eos = tj.get("eos_token_id", 49407)
    return tcfg, vcfg, (None if eos == 2 else int(eos))


class HipClipScorer:
    """uint8 images + prompts -> per-pair CLIP score, both towers on libsdhip."""

    def __init__(self, text_model: HipClipTextModel, vision_model: HipClipVisionModel, tokenizer: ClipBpeTokenizer):
        self.text_model, self.vision_model, self.tokenizer = text_model, vision_model, tokenizer

    @classmethod
    def from_pretrained(cls, model_dir: str, device=None) -> "HipClipScorer":
        """``device``: where both towers live and run (``None``: the current device); the process's current device is
        left as it is."""
        tcfg, vcfg, eos = read_clip_configs(model_dir)          # config errors before any GPU work
        from safetensors.torch import load_file
        path = os.path.join(model_dir, "model.safetensors")
        if not os.path.isfile(path):
            raise FileNotFoundError(f"no model.safetensors under {model_dir!r}")
        sd = {k: v.float() for k, v in load_file(path).items() if not k.endswith("position_ids")}
        text_sd = {k: v for k, v in sd.items() if k.startswith("text_model.")}
        if "text_projection.weight" not in sd:
            raise KeyError("checkpoint lacks text_projection.weight")
        tok_kw = {}
        tc = os.path.join(model_dir, "tokenizer_config.json")
        if os.path.isfile(tc):
            pad = _read_json(tc).get("pad_token")
            if isinstance(pad, dict):
                pad = pad.get("content")
            if pad:
                tok_kw["pad_token"] = pad
        tok = ClipBpeTokenizer.from_pretrained(model_dir, model_max_length=tcfg.max_position_embeddings, **tok_kw)
        device = resolve_device(device)
        text = HipClipTextModel(tcfg, text_sd, device=device, text_projection=sd["text_projection.weight"], eos_token_id=eos)
        vision = HipClipVisionModel(vcfg, sd, device=device)
        return cls(text, vision, tok)

    def text_embeds(self, prompts: Sequence[str]) -> torch.Tensor:
        # Every prompt is padded to max_position_embeddings, where the processor pads to the longest prompt
        # (padding=True): the text tower's mask is causal, so the positions after EOS never reach the EOS row, and the
        # pooled row is the same either way.
        return self.text_model.embeds(self.tokenizer(list(prompts)))

    def image_embeds(self, images) -> torch.Tensor:
        """uint8 ``[B,3,H,W]`` or a list of uint8 ``[3,H,W]`` (sizes may differ: same-size images run as one batch)."""
        if torch.is_tensor(images):
            return self.vision_model.encode(images)
        images = list(images)
        out: List[Optional[torch.Tensor]] = [None] * len(images)
        groups: Dict[tuple, List[int]] = {}
        for i, im in enumerate(images):
            groups.setdefault(tuple(im.shape), []).append(i)
        for idx in groups.values():
            emb = self.vision_model.encode(torch.stack([images[i] for i in idx]))
            for j, i in enumerate(idx):
                out[i] = emb[j]
        return torch.stack(out)

    def score_pairs(self, images, prompts: Sequence[str]) -> Tuple[torch.Tensor, torch.Tensor]:
        """``(raw, score)`` per pair: ``100 cos(img, txt)`` and ``max(raw, 0)`` (fp32, on the GPU)."""
        if len(prompts) != len(images):
            raise ValueError(f"{len(images)} images but {len(prompts)} prompts")
        return clip_score_pairs(self.image_embeds(images), self.text_embeds(prompts))
