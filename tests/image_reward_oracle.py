"""fp32 CPU oracle of ImageReward (test infrastructure, like tests/clip_vision_oracle.py): a PyTorch restatement of what
``sonicdiffusionbayeslab_amd.image_reward`` computes on the GPU, over a state dict under the CHECKPOINT's keys.

* ``vision_forward``  -- BLIP's ViT: patch conv WITH bias, class token, position embedding, no pre-LayerNorm, pre-LN blocks
                         with the fused qkv and the exact GELU, the final ``norm`` over all tokens -> [B, tokens, H_v].
* ``text_forward``    -- BLIP's BERT in multimodal mode: word + position embedding and LayerNorm, post-LN layers with
                         self-attention under the key-padding mask (additive -10000, as upstream's extended mask),
                         cross-attention over the image tokens (no mask) and a GELU MLP -> last_hidden_state.
* ``reward_head``     -- the five Linears one after the other, then (r - mean) / std.
* ``score`` / ``inference_rank`` -- preprocessing (tests/clip_vision_oracle.pil_crop: Pillow bicubic, centre crop, CLIP mean
                         and std), tokenisation with the package's tokenizer, features and rewards.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from tests.clip_vision_oracle import pil_crop, pixel_values


def _lin(sd, n, x):
    return F.linear(x, sd[n + ".weight"].float(), sd[n + ".bias"].float())


def _ln(sd, n, x, eps):
    return F.layer_norm(x, (x.shape[-1],), sd[n + ".weight"].float(), sd[n + ".bias"].float(), eps)


def _heads(t, heads):
    B, L, H = t.shape
    return t.view(B, L, heads, H // heads).transpose(1, 2)


def _attend(q, k, v, heads, bias=None):
    d = q.shape[-1] // heads
    s = _heads(q, heads) @ _heads(k, heads).transpose(-1, -2) / d ** 0.5
    if bias is not None:
        s = s + bias
    a = torch.softmax(s, dim=-1) @ _heads(v, heads)
    return a.transpose(1, 2).reshape(q.shape)


@torch.no_grad()
def vision_forward(sd, cfg, pix: torch.Tensor) -> torch.Tensor:
    p = "blip.visual_encoder."
    H, eps, heads = cfg.vision_hidden_size, cfg.vision_layer_norm_eps, cfg.vision_num_attention_heads
    x = F.conv2d(pix.float(), sd[p + "patch_embed.proj.weight"].float(), sd[p + "patch_embed.proj.bias"].float(),
                 stride=cfg.patch_size).flatten(2).transpose(1, 2)
    B = x.shape[0]
    h = torch.cat([sd[p + "cls_token"].float().expand(B, 1, H), x], 1) + sd[p + "pos_embed"].float()
    for i in range(cfg.vision_num_hidden_layers):
        b = f"{p}blocks.{i}."
        q, k, v = _lin(sd, b + "attn.qkv", _ln(sd, b + "norm1", h, eps)).chunk(3, dim=-1)
        h = h + _lin(sd, b + "attn.proj", _attend(q, k, v, heads))
        h = h + _lin(sd, b + "mlp.fc2", F.gelu(_lin(sd, b + "mlp.fc1", _ln(sd, b + "norm2", h, eps))))
    return _ln(sd, p + "norm", h, eps)


@torch.no_grad()
def text_forward(sd, cfg, ids: torch.Tensor, mask: torch.Tensor, image_tokens: torch.Tensor) -> torch.Tensor:
    p = "blip.text_encoder."
    eps, heads = cfg.layer_norm_eps, cfg.num_attention_heads
    L = ids.shape[1]
    h = sd[p + "embeddings.word_embeddings.weight"].float()[ids.long()] + sd[p + "embeddings.position_embeddings.weight"].float()[:L]
    h = _ln(sd, p + "embeddings.LayerNorm", h, eps)
    bias = (1.0 - mask.float())[:, None, None, :] * -10000.0
    for i in range(cfg.num_hidden_layers):
        l = f"{p}encoder.layer.{i}."
        a = _attend(_lin(sd, l + "attention.self.query", h), _lin(sd, l + "attention.self.key", h),
                    _lin(sd, l + "attention.self.value", h), heads, bias)
        h = _ln(sd, l + "attention.output.LayerNorm", h + _lin(sd, l + "attention.output.dense", a), eps)
        a = _attend(_lin(sd, l + "crossattention.self.query", h), _lin(sd, l + "crossattention.self.key", image_tokens),
                    _lin(sd, l + "crossattention.self.value", image_tokens), heads)
        h = _ln(sd, l + "crossattention.output.LayerNorm", h + _lin(sd, l + "crossattention.output.dense", a), eps)
        f = F.gelu(_lin(sd, l + "intermediate.dense", h))
        h = _ln(sd, l + "output.LayerNorm", h + _lin(sd, l + "output.dense", f), eps)
    return h


@torch.no_grad()
def reward_head(sd, cfg, feats: torch.Tensor) -> torch.Tensor:
    x = feats.float()
    for k in (0, 2, 4, 6, 7):
        x = _lin(sd, f"mlp.layers.{k}", x)
    return (x[:, 0] - cfg.reward_mean) / cfg.reward_std


def preprocess(images, cfg) -> torch.Tensor:
    return torch.stack([pixel_values(pil_crop(im.cpu(), cfg.image_size)) for im in images])


@torch.no_grad()
def features(sd, cfg, tokenizer, prompts, images) -> torch.Tensor:
    prompts = [prompts] * len(images) if isinstance(prompts, str) else list(prompts)
    ids, mask = tokenizer(prompts)
    return features_from_ids(sd, cfg, ids, mask, images)


@torch.no_grad()
def features_from_ids(sd, cfg, ids, mask, images) -> torch.Tensor:
    tokens = vision_forward(sd, cfg, preprocess(images, cfg))
    return text_forward(sd, cfg, ids, mask, tokens)[:, 0]


def score(sd, cfg, tokenizer, prompts, images) -> torch.Tensor:
    return reward_head(sd, cfg, features(sd, cfg, tokenizer, prompts, images))


def inference_rank(sd, cfg, tokenizer, prompt: str, images):
    rewards = score(sd, cfg, tokenizer, prompt, images)
    order = torch.sort(rewards, descending=True).indices
    return (torch.sort(order).indices + 1).tolist(), rewards.tolist()
