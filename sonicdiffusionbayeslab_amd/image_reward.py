"""ImageReward on libsdhip: the reference's third quality metric (``quality_metrics.image_reward``,
``src/metrics/metrics.py:44-95``: ``ImageReward-v1.0`` scores a generated image and the dataset's real one against the prompt).

ImageReward-v1.0 is BLIP's ViT-L/16 (timm layout), BLIP's BERT text encoder whose layers cross-attend to the image tokens, and
a five-Linear reward head on the class-token row, ``(r - mean) / std``.  Everything from the uint8 image to the reward runs in
libsdhip (``sd_image_reward_create`` / ``sd_image_reward_score``); tokenisation is host-side text processing.

* ``BertWordPieceTokenizer`` -- ``bert-base-uncased`` WordPiece over a ``vocab.txt`` (BasicTokenizer + greedy longest match),
  ``[CLS] ... [SEP]`` padded with id 0 to ``max_length``.
* ``ImageRewardConfig`` / ``read_image_reward_dir`` -- a LOCAL directory with ``ImageReward.pt`` or ``.safetensors``,
  ``med_config.json``, ``vocab.txt`` and optionally ``vision_config.json`` (default: ViT-L/16).
* ``image_reward_name_table`` -- the ONE table from checkpoint keys to the library's parameter names and shapes.  The
  ``image-reward`` package is not available offline: every key in it is restated from memory of ``image-reward==1.5`` and is
  corrected here, nowhere else, when a real checkpoint disagrees.
* ``HipImageReward`` -- ``score`` / ``inference_rank`` / ``features``.
"""
from __future__ import annotations

import ctypes as C
import json
import math
import os
import unicodedata
from dataclasses import dataclass
from typing import Dict, List, Sequence, Tuple

import torch

from . import _lib
from .handle import HipHandle, Workspace, load_params

REWARD_MEAN, REWARD_STD = 0.16717362830052426, 1.0333394966054072
HEAD_LAYERS = (0, 2, 4, 6, 7)                    # mlp.layers.N that are Linears (the others are Dropouts)
HEAD_DIMS = (1024, 128, 64, 16, 1)
MAX_IMAGE_TOKENS, MAX_TEXT_LEN, MAX_HIDDEN = 320, 64, 1536


# ---------------------------------------------------------------------------------------------------------------------
# tokenizer
# ---------------------------------------------------------------------------------------------------------------------

def _is_whitespace(ch: str) -> bool:
    return ch in " \t\n\r" or unicodedata.category(ch) == "Zs"


def _is_control(ch: str) -> bool:
    return ch not in "\t\n\r" and unicodedata.category(ch).startswith("C")


def _is_punctuation(ch: str) -> bool:
    cp = ord(ch)
    if 33 <= cp <= 47 or 58 <= cp <= 64 or 91 <= cp <= 96 or 123 <= cp <= 126:
        return True
    return unicodedata.category(ch).startswith("P")


def _is_cjk(cp: int) -> bool:
    return (0x4E00 <= cp <= 0x9FFF or 0x3400 <= cp <= 0x4DBF or 0x20000 <= cp <= 0x2A6DF or 0x2A700 <= cp <= 0x2B73F or
            0x2B740 <= cp <= 0x2B81F or 0x2B820 <= cp <= 0x2CEAF or 0xF900 <= cp <= 0xFAFF or 0x2F800 <= cp <= 0x2FA1F)


class BertWordPieceTokenizer:
    """transformers ``BertTokenizer`` for an uncased vocabulary: clean the text, space out CJK characters, lower-case, strip
    accents (NFD, drop Mn), split on whitespace and punctuation, then WordPiece (greedy longest match, ``##`` continuation, a
    word of more than 100 characters -> ``[UNK]``)."""

    def __init__(self, vocab: Dict[str, int], max_length: int = 35, max_input_chars_per_word: int = 100):
        for t in ("[PAD]", "[UNK]", "[CLS]", "[SEP]"):
            if t not in vocab:
                raise KeyError(f"vocab.txt lacks the special token {t}")
        self.vocab, self.max_length, self.max_chars = vocab, int(max_length), max_input_chars_per_word
        self.pad_id, self.unk_id, self.cls_id, self.sep_id = (vocab[t] for t in ("[PAD]", "[UNK]", "[CLS]", "[SEP]"))

    @classmethod
    def from_file(cls, path: str, max_length: int = 35) -> "BertWordPieceTokenizer":
        with open(path, encoding="utf-8") as f:
            vocab = {line.rstrip("\n"): i for i, line in enumerate(f)}
        return cls(vocab, max_length)

    def basic_tokens(self, text: str) -> List[str]:
        out = []
        for ch in text:
            cp = ord(ch)
            if cp == 0 or cp == 0xFFFD or _is_control(ch):
                continue
            if _is_whitespace(ch):
                out.append(" ")
            elif _is_cjk(cp):
                out.append(f" {ch} ")
            else:
                out.append(ch)
        words = []
        for tok in "".join(out).split():
            tok = "".join(c for c in unicodedata.normalize("NFD", tok.lower()) if unicodedata.category(c) != "Mn")
            cur = ""
            for ch in tok:
                if _is_punctuation(ch):
                    if cur:
                        words.append(cur)
                    words.append(ch)
                    cur = ""
                else:
                    cur += ch
            if cur:
                words.append(cur)
        return words

    def wordpiece(self, word: str) -> List[int]:
        if len(word) > self.max_chars:
            return [self.unk_id]
        ids, start = [], 0
        while start < len(word):
            end, cur = len(word), None
            while start < end:
                sub = ("##" if start else "") + word[start:end]
                if sub in self.vocab:
                    cur = self.vocab[sub]
                    break
                end -= 1
            if cur is None:
                return [self.unk_id]
            ids.append(cur)
            start = end
        return ids

    def encode(self, text: str) -> List[int]:
        """``[CLS] pieces [SEP]`` truncated to ``max_length`` (the ``[SEP]`` stays), without padding."""
        ids = [i for w in self.basic_tokens(text) for i in self.wordpiece(w)]
        return [self.cls_id] + ids[:self.max_length - 2] + [self.sep_id]

    def __call__(self, prompts: Sequence[str]) -> Tuple[torch.Tensor, torch.Tensor]:
        """``(input_ids, attention_mask)``, int32 ``[B, max_length]``, padded with id 0 (``padding='max_length'``)."""
        ids = torch.full((len(prompts), self.max_length), self.pad_id, dtype=torch.int32)
        mask = torch.zeros_like(ids)
        for b, p in enumerate(prompts):
            e = self.encode(p)
            ids[b, :len(e)] = torch.tensor(e, dtype=torch.int32)
            mask[b, :len(e)] = 1
        return ids, mask


# ---------------------------------------------------------------------------------------------------------------------
# config, names, synthetic weights
# ---------------------------------------------------------------------------------------------------------------------

@dataclass
class ImageRewardConfig:
    # BLIP ViT-L/16 (BLIP's vit.py over timm's VisionTransformer)
    vision_hidden_size: int = 1024
    vision_num_hidden_layers: int = 24
    vision_num_attention_heads: int = 16
    vision_intermediate_size: int = 4096
    image_size: int = 224
    patch_size: int = 16
    vision_layer_norm_eps: float = 1e-6
    # BLIP med_config.json (encoder_width is the vision width: BLIP sets it from the tower it builds)
    vocab_size: int = 30524
    hidden_size: int = 768
    num_hidden_layers: int = 12
    num_attention_heads: int = 12
    intermediate_size: int = 3072
    max_position_embeddings: int = 512
    layer_norm_eps: float = 1e-12
    hidden_act: str = "gelu"
    position_embedding_type: str = "absolute"
    max_text_len: int = 35
    reward_mean: float = REWARD_MEAN
    reward_std: float = REWARD_STD

    @property
    def image_tokens(self) -> int:
        return (self.image_size // self.patch_size) ** 2 + 1


def check_image_reward_config(cfg: ImageRewardConfig) -> None:
    """The shapes libsdhip builds; ``ValueError`` naming the field otherwise (raised before any GPU work)."""
    for f in ("vision_hidden_size", "hidden_size"):
        v = getattr(cfg, f)
        if v <= 0 or v % 64 or v > MAX_HIDDEN:
            raise ValueError(f"{f}={v}: a multiple of 64 up to {MAX_HIDDEN} is built")
    for f in ("vision_intermediate_size", "intermediate_size"):
        v = getattr(cfg, f)
        if v <= 0 or v % 64:
            raise ValueError(f"{f}={v}: a positive multiple of 64 is built")
    for f, h in (("vision_num_attention_heads", cfg.vision_hidden_size), ("num_attention_heads", cfg.hidden_size)):
        v = getattr(cfg, f)
        if v <= 0 or h != 64 * v:
            raise ValueError(f"{f}={v}: head dim 64 is built (hidden size {h})")
    if cfg.patch_size <= 0 or cfg.image_size < cfg.patch_size or cfg.image_size % cfg.patch_size:
        raise ValueError(f"patch_size={cfg.patch_size} must divide image_size={cfg.image_size}")
    if cfg.image_tokens > MAX_IMAGE_TOKENS:
        raise ValueError(f"image_size={cfg.image_size}: {cfg.image_tokens} image tokens (at most {MAX_IMAGE_TOKENS} are built)")
    if not 1 <= cfg.max_text_len <= min(MAX_TEXT_LEN, cfg.max_position_embeddings):
        raise ValueError(f"max_text_len={cfg.max_text_len}: 1..{MAX_TEXT_LEN} (and at most max_position_embeddings) is built")
    if cfg.hidden_act != "gelu":
        raise ValueError(f"hidden_act={cfg.hidden_act!r}: only 'gelu' is built")
    if cfg.position_embedding_type != "absolute":
        raise ValueError(f"position_embedding_type={cfg.position_embedding_type!r}: only 'absolute' is built")
    for f in ("vision_num_hidden_layers", "num_hidden_layers", "vocab_size"):
        if getattr(cfg, f) < 1:
            raise ValueError(f"{f}={getattr(cfg, f)} must be positive")
    for f in ("vision_layer_norm_eps", "layer_norm_eps", "reward_std"):
        if not getattr(cfg, f) > 0:
            raise ValueError(f"{f}={getattr(cfg, f)} must be positive")


def image_reward_param_shapes(cfg: ImageRewardConfig) -> List[Tuple[str, Tuple[int, ...]]]:
    """The library's parameter names (BLIP's own, without the checkpoint's ``blip.`` prefix) and shapes, in module order."""
    VH, VI, P = cfg.vision_hidden_size, cfg.vision_intermediate_size, cfg.patch_size
    H, I = cfg.hidden_size, cfg.intermediate_size
    out: List[Tuple[str, Tuple[int, ...]]] = []

    def lin(n, o, i):
        out.append((n + ".weight", (o, i))); out.append((n + ".bias", (o,)))

    def norm(n, h):
        out.append((n + ".weight", (h,))); out.append((n + ".bias", (h,)))

    out.append(("visual_encoder.cls_token", (VH,)))
    out.append(("visual_encoder.pos_embed", (cfg.image_tokens, VH)))
    out.append(("visual_encoder.patch_embed.proj.weight", (VH, 3, P, P)))
    out.append(("visual_encoder.patch_embed.proj.bias", (VH,)))
    for i in range(cfg.vision_num_hidden_layers):
        p = f"visual_encoder.blocks.{i}."
        norm(p + "norm1", VH); lin(p + "attn.qkv", 3 * VH, VH); lin(p + "attn.proj", VH, VH)
        norm(p + "norm2", VH); lin(p + "mlp.fc1", VI, VH); lin(p + "mlp.fc2", VH, VI)
    norm("visual_encoder.norm", VH)
    out.append(("text_encoder.embeddings.word_embeddings.weight", (cfg.vocab_size, H)))
    out.append(("text_encoder.embeddings.position_embeddings.weight", (cfg.max_position_embeddings, H)))
    norm("text_encoder.embeddings.LayerNorm", H)
    for i in range(cfg.num_hidden_layers):
        p = f"text_encoder.encoder.layer.{i}."
        for n in ("query", "key", "value"):
            lin(p + "attention.self." + n, H, H)
        lin(p + "attention.output.dense", H, H); norm(p + "attention.output.LayerNorm", H)
        lin(p + "crossattention.self.query", H, H)
        lin(p + "crossattention.self.key", H, VH); lin(p + "crossattention.self.value", H, VH)
        lin(p + "crossattention.output.dense", H, H); norm(p + "crossattention.output.LayerNorm", H)
        lin(p + "intermediate.dense", I, H); lin(p + "output.dense", H, I); norm(p + "output.LayerNorm", H)
    fan = H
    for k, d in zip(HEAD_LAYERS, HEAD_DIMS):
        lin(f"mlp.layers.{k}", d, fan)
        fan = d
    return out


def image_reward_name_table(cfg: ImageRewardConfig) -> List[Tuple[str, str, Tuple[int, ...], Tuple[int, ...]]]:
    """``(checkpoint key, library name, checkpoint shape, library shape)`` for every parameter: the towers sit under ``blip.``
    in ``ImageReward.pt``, the head under ``mlp.``; timm keeps ``cls_token`` as ``[1,1,H]`` and ``pos_embed`` as
    ``[1,tokens,H]``.  UNPINNED: restated from memory of ``image-reward==1.5`` (see the module docstring)."""
    table = []
    for name, shape in image_reward_param_shapes(cfg):
        up_shape = shape
        if name == "visual_encoder.cls_token":
            up_shape = (1, 1) + shape
        elif name == "visual_encoder.pos_embed":
            up_shape = (1,) + shape
        table.append((name if name.startswith("mlp.") else "blip." + name, name, up_shape, shape))
    return table


def map_image_reward_state_dict(cfg: ImageRewardConfig, sd: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """Checkpoint state dict -> the library's names and shapes (fp32, host); ``KeyError`` / ``ValueError`` name the key."""
    out = {}
    for up, name, up_shape, shape in image_reward_name_table(cfg):
        if up not in sd:
            raise KeyError(f"ImageReward checkpoint lacks {up!r}")
        t = sd[up]
        if tuple(t.shape) != tuple(up_shape):
            raise ValueError(f"{up}: expected shape {tuple(up_shape)}, got {tuple(t.shape)}")
        out[name] = t.detach().to("cpu", torch.float32).reshape(shape).contiguous()
    return out


def make_synthetic_image_reward_state_dict(cfg: ImageRewardConfig, seed: int = 909) -> Dict[str, torch.Tensor]:
    """Seeded ImageReward-shaped weights under the CHECKPOINT's keys, on the bf16 grid (no ImageReward weights exist offline)."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for up, name, up_shape, _ in image_reward_name_table(cfg):
        if name.endswith("patch_embed.proj.weight"):
            t = torch.randn(up_shape, generator=g) / math.sqrt(up_shape[1] * up_shape[2] * up_shape[3])
        elif name.endswith("cls_token") or name.endswith("pos_embed"):
            t = torch.randn(up_shape, generator=g) * 0.1
        elif "embeddings.word" in name or "embeddings.position" in name:
            t = torch.randn(up_shape, generator=g) * (0.5 if "word" in name else 0.25)
        elif name.endswith(".bias"):
            t = torch.randn(up_shape, generator=g) * 0.02
        elif "norm" in name.lower():
            t = 1.0 + 0.1 * torch.randn(up_shape, generator=g)
        else:
            t = torch.randn(up_shape, generator=g) / math.sqrt(up_shape[1])
        sd[up] = t.to(torch.bfloat16).float()
    return sd


def fold_reward_head(sd: Dict[str, torch.Tensor], prefix: str = "mlp.layers.") -> Tuple[torch.Tensor, float]:
    """The five Linears as ONE ``(w [H], b)`` in fp64: there is no activation between them and the Dropouts are identity in
    eval mode, so ``r = W7 (W6 (W4 (W2 (W0 x + b0) + b2) + b4) + b6) + b7 = w . x + b`` (libsdhip folds the same way at
    finalize)."""
    w = torch.ones(1, 1, dtype=torch.float64)
    b = torch.zeros(1, dtype=torch.float64)
    for k in reversed(HEAD_LAYERS):
        W, B = sd[f"{prefix}{k}.weight"].double(), sd[f"{prefix}{k}.bias"].double()
        b = b + w @ B
        w = w @ W
    return w[0], float(b)


def _read_json(path: str) -> dict:
    with open(path, encoding="utf-8") as f:
        return json.load(f)


def read_image_reward_dir(model_dir: str) -> Tuple[ImageRewardConfig, str, str]:
    """``(config, weights path, vocab path)`` of a local ImageReward directory; unsupported fields raise ``ValueError``."""
    if not os.path.isdir(model_dir):
        raise FileNotFoundError(f"ImageReward directory {model_dir!r} does not exist")
    med = os.path.join(model_dir, "med_config.json")
    vocab = os.path.join(model_dir, "vocab.txt")
    for p in (med, vocab):
        if not os.path.isfile(p):
            raise FileNotFoundError(f"no {os.path.basename(p)} under {model_dir!r}")
    weights = next((os.path.join(model_dir, n) for n in ("ImageReward.safetensors", "ImageReward.pt")
                    if os.path.isfile(os.path.join(model_dir, n))), None)
    if weights is None:
        raise FileNotFoundError(f"no ImageReward.pt or ImageReward.safetensors under {model_dir!r}")
    kw = {}
    mj = _read_json(med)
    for k in ("vocab_size", "hidden_size", "num_hidden_layers", "num_attention_heads", "intermediate_size",
              "max_position_embeddings", "layer_norm_eps", "hidden_act", "position_embedding_type"):
        if k in mj:
            kw[k] = mj[k]
    vc = os.path.join(model_dir, "vision_config.json")
    if os.path.isfile(vc):
        vj = _read_json(vc)
        for k, f in (("hidden_size", "vision_hidden_size"), ("num_hidden_layers", "vision_num_hidden_layers"),
                     ("num_attention_heads", "vision_num_attention_heads"), ("intermediate_size", "vision_intermediate_size"),
                     ("image_size", "image_size"), ("patch_size", "patch_size"), ("layer_norm_eps", "vision_layer_norm_eps"),
                     ("max_text_len", "max_text_len"), ("reward_mean", "reward_mean"), ("reward_std", "reward_std")):
            if k in vj:
                kw[f] = vj[k]
    cfg = ImageRewardConfig(**kw)
    check_image_reward_config(cfg)
    return cfg, weights, vocab


def load_image_reward_weights(path: str) -> Dict[str, torch.Tensor]:
    if path.endswith(".safetensors"):
        from safetensors.torch import load_file
        return dict(load_file(path))
    sd = torch.load(path, map_location="cpu", weights_only=True)
    return sd.get("state_dict", sd) if isinstance(sd, dict) else sd


# ---------------------------------------------------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------------------------------------------------

class HipImageReward(HipHandle):
    """``ImageReward.score`` / ``inference_rank`` on libsdhip: uint8 images + prompts -> rewards."""

    def __init__(self, config: ImageRewardConfig, state_dict: Dict[str, torch.Tensor], tokenizer: BertWordPieceTokenizer,
                 device=None):
        """``state_dict`` under the checkpoint's keys.  ``device``: where the weights live and the model runs (``None``: the
        current device); the process's current device is left as it is."""
        check_image_reward_config(config)
        params = map_image_reward_state_dict(config, state_dict)       # key / shape errors before any GPU work
        if tokenizer.max_length != config.max_text_len:
            raise ValueError(f"tokenizer max_length {tokenizer.max_length} != max_text_len {config.max_text_len}")
        super().__init__(device, resolve=True)
        self.config, self.tokenizer = config, tokenizer
        self._sized = None                  # the (batch, H, W) the workspace was last sized for (grow-only: it may be larger)
        with torch.cuda.device(self.device):
            self._build(config, params)

    def _build(self, cfg: ImageRewardConfig, params: Dict[str, torch.Tensor]) -> None:
        c = _lib.SdImageRewardConfig(
            cfg.vision_hidden_size, cfg.vision_num_hidden_layers, cfg.vision_num_attention_heads, cfg.vision_intermediate_size,
            cfg.image_size, cfg.patch_size, cfg.vision_layer_norm_eps, cfg.vocab_size, cfg.hidden_size, cfg.num_hidden_layers,
            cfg.num_attention_heads, cfg.intermediate_size, cfg.max_position_embeddings, cfg.layer_norm_eps, 1, 1,
            cfg.max_text_len, cfg.reward_mean, cfg.reward_std)
        _lib.check(self._lib.sd_image_reward_create(C.byref(c), C.byref(self._handle)), "sd_image_reward_create")
        load_params(self._lib, self._handle, image_reward_param_shapes(cfg), params, "ImageReward")
        self._finalize()

    @classmethod
    def from_pretrained(cls, model_dir: str, device=None) -> "HipImageReward":
        cfg, weights, vocab = read_image_reward_dir(model_dir)           # config errors before any GPU work
        tok = BertWordPieceTokenizer.from_file(vocab, max_length=cfg.max_text_len)
        return cls(cfg, load_image_reward_weights(weights), tok, device=device)

    def _score_batch(self, images: torch.Tensor, ids: torch.Tensor, mask: torch.Tensor):
        if images.dtype != torch.uint8 or images.dim() != 4 or images.shape[1] != 3:
            raise ValueError(f"images must be uint8 [B,3,H,W], got {images.dtype} {tuple(images.shape)}")
        x = images.to(self.device).contiguous()
        b, _, h, w = x.shape
        L = ids.shape[1]
        ids = ids.to(self.device, torch.int32).contiguous()
        mask = mask.to(self.device, torch.int32).contiguous()
        if self._sized != (b, h, w):
            self._wsp.reserve(Workspace.bytes_or_raise(self._lib.sd_image_reward_workspace_bytes(self._handle, b, h, w),
                                                       "sd_image_reward_workspace_bytes"))
            self._sized = (b, h, w)
        rewards = torch.empty(b, dtype=torch.float32, device=self.device)
        feats = torch.empty((b, self.config.hidden_size), dtype=torch.float32, device=self.device)
        _lib.check(self._lib.sd_image_reward_score(self._handle, _lib.current_stream(), x.data_ptr(), ids.data_ptr(),
                                                   mask.data_ptr(), b, L, h, w, rewards.data_ptr(), feats.data_ptr(), self._wsp.ptr,
                                                   self._wsp.nbytes), "sd_image_reward_score")
        return rewards, feats

    def _run(self, prompts, images) -> Tuple[torch.Tensor, torch.Tensor]:
        n = images.shape[0] if torch.is_tensor(images) else len(images)
        prompts = [prompts] * n if isinstance(prompts, str) else list(prompts)
        if len(prompts) != n:
            raise ValueError(f"{n} images but {len(prompts)} prompts")
        if n == 0:
            raise ValueError("no images to score")
        ids, mask = self.tokenizer(prompts)
        with torch.cuda.device(self.device):
            if torch.is_tensor(images):
                return self._score_batch(images, ids, mask)
            images = list(images)
            groups: Dict[tuple, List[int]] = {}
            for i, im in enumerate(images):
                groups.setdefault(tuple(im.shape), []).append(i)
            rewards = torch.empty(n, dtype=torch.float32, device=self.device)
            feats = torch.empty((n, self.config.hidden_size), dtype=torch.float32, device=self.device)
            for idx in groups.values():       # same-size images run as one batch
                sel = torch.tensor(idx)
                r, f = self._score_batch(torch.stack([images[i] for i in idx]), ids[sel], mask[sel])
                rewards[sel.to(self.device)] = r
                feats[sel.to(self.device)] = f
            return rewards, feats

    def score(self, prompts, images) -> torch.Tensor:
        """Rewards, fp32 ``[B]`` on the GPU.  ``prompts``: one per image, or one string for all.  ``images``: uint8
        ``[B,3,H,W]`` or a list of uint8 ``[3,H,W]`` (sizes may differ)."""
        return self._run(prompts, images)[0]

    def features(self, prompts, images) -> torch.Tensor:
        """``last_hidden_state[:, 0]`` of the text encoder, fp32 ``[B, hidden_size]``: what the reward head reads."""
        return self._run(prompts, images)[1]

    def inference_rank(self, prompt: str, images) -> Tuple[List[int], List[float]]:
        """``(ranks, rewards)`` as upstream's ``inference_rank``: rank 1 for the largest reward."""
        rewards = self.score(prompt, images).cpu()
        order = torch.sort(rewards, descending=True).indices
        ranks = torch.sort(order).indices + 1
        return ranks.tolist(), rewards.tolist()
