"""fp32 CPU oracle of the CLIP score path (test infrastructure, like tests/cond_oracle.py).

* ``pil_crop``            -- CLIPImageProcessor's geometry on one uint8 [3,H,W] image with Pillow: resize the shortest edge
                             to S (long edge int(S * long / short)) with BICUBIC, centre crop (top = (h - S) // 2).
* ``pixel_values``        -- the crop normalised, (x / 255 - mean) / std (what CLIPImageProcessor hands the model).
* ``clip_vision_forward`` -- CLIPVisionModelWithProjection(pixel_values).image_embeds restated in torch: patch embedding
                             (no bias), class token, position embedding, pre_layrnorm, pre-LN layers with non-causal
                             attention and quick_gelu, post_layernorm of the class token, visual_projection (no bias).
* ``clip_text_embeds``    -- oracle/clip.py's text tower, the pooled EOS row (argmax of the ids, or the first eos id),
                             text_projection.
* ``clip_scores``         -- 100 cos per pair (unclamped).
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

MEAN = torch.tensor([0.48145466, 0.4578275, 0.40821073])
STD = torch.tensor([0.26862954, 0.26130258, 0.27577711])


def resize_geometry(h, w, S):
    if w <= h:
        rw, rh = S, int(S * h / w)
    else:
        rh, rw = S, int(S * w / h)
    return rh, rw, (rh - S) // 2, (rw - S) // 2


def pil_crop(img: torch.Tensor, S: int) -> torch.Tensor:
    """uint8 [3,H,W] -> uint8 [3,S,S] through PIL.Image.resize(BICUBIC) and the centre crop."""
    from PIL import Image
    _, h, w = img.shape
    rh, rw, top, left = resize_geometry(h, w, S)
    im = Image.fromarray(img.permute(1, 2, 0).contiguous().numpy(), "RGB").resize((rw, rh), Image.BICUBIC)
    a = np.asarray(im)[top:top + S, left:left + S]
    return torch.from_numpy(a.copy()).permute(2, 0, 1).contiguous()


def pixel_values(crop: torch.Tensor) -> torch.Tensor:
    return (crop.float() / 255.0 - MEAN[:, None, None]) / STD[:, None, None]


def quick_gelu(x):
    return x * torch.sigmoid(1.702 * x)


def _encoder(h, w, prefix, n_layers, heads, eps, causal):
    B, L, H = h.shape
    d = H // heads
    P = lambda n: w[prefix + n].float()
    mask = torch.full((L, L), float("-inf")).triu(1) if causal else torch.zeros(L, L)
    for i in range(n_layers):
        p = f"encoder.layers.{i}."
        r = h
        x = F.layer_norm(h, (H,), P(p + "layer_norm1.weight"), P(p + "layer_norm1.bias"), eps)
        q = F.linear(x, P(p + "self_attn.q_proj.weight"), P(p + "self_attn.q_proj.bias")) * d ** -0.5
        k = F.linear(x, P(p + "self_attn.k_proj.weight"), P(p + "self_attn.k_proj.bias"))
        v = F.linear(x, P(p + "self_attn.v_proj.weight"), P(p + "self_attn.v_proj.bias"))
        sp = lambda t: t.view(B, L, heads, d).transpose(1, 2)
        a = torch.softmax(sp(q) @ sp(k).transpose(-1, -2) + mask, dim=-1) @ sp(v)
        h = r + F.linear(a.transpose(1, 2).reshape(B, L, H), P(p + "self_attn.out_proj.weight"), P(p + "self_attn.out_proj.bias"))
        r = h
        x = F.layer_norm(h, (H,), P(p + "layer_norm2.weight"), P(p + "layer_norm2.bias"), eps)
        h = r + F.linear(quick_gelu(F.linear(x, P(p + "mlp.fc1.weight"), P(p + "mlp.fc1.bias"))),
                         P(p + "mlp.fc2.weight"), P(p + "mlp.fc2.bias"))
    return h


@torch.no_grad()
def clip_vision_forward(w, cfg, pix: torch.Tensor) -> torch.Tensor:
    """image_embeds [B, projection_dim] from pixel_values [B,3,S,S]; ``cfg`` a clip_score.ClipVisionConfig."""
    P = lambda n: w["vision_model." + n].float()
    x = F.conv2d(pix.float(), P("embeddings.patch_embedding.weight"), stride=cfg.patch_size)     # [B, H, G, G]
    B, H = x.shape[:2]
    x = x.flatten(2).transpose(1, 2)
    h = torch.cat([P("embeddings.class_embedding").expand(B, 1, H), x], 1) + P("embeddings.position_embedding.weight")
    h = F.layer_norm(h, (H,), P("pre_layrnorm.weight"), P("pre_layrnorm.bias"), cfg.layer_norm_eps)
    h = _encoder(h, w, "vision_model.", cfg.num_hidden_layers, cfg.num_attention_heads, cfg.layer_norm_eps, causal=False)
    pooled = F.layer_norm(h[:, 0], (H,), P("post_layernorm.weight"), P("post_layernorm.bias"), cfg.layer_norm_eps)
    return F.linear(pooled, w["visual_projection.weight"].float())


@torch.no_grad()
def clip_text_embeds(w, cfg, ids: torch.Tensor, eos_token_id=None) -> torch.Tensor:
    """text_embeds [B, projection_dim]; ``cfg`` a clip.ClipTextConfig; eos_token_id None: pool at argmax(ids)."""
    from oracle.clip import ClipTextConfig as OC, clip_text_forward
    kw = {k: getattr(cfg, k) for k in ("vocab_size", "hidden_size", "num_hidden_layers", "num_attention_heads",
                                        "intermediate_size", "max_position_embeddings", "layer_norm_eps")}
    tw = {k: v for k, v in w.items() if k.startswith("text_model.")}
    h = clip_text_forward(tw, OC(**kw), ids.long())
    pos = ids.long().argmax(-1) if eos_token_id is None else (ids.long() == eos_token_id).int().argmax(-1)
    return F.linear(h[torch.arange(h.shape[0]), pos], w["text_projection.weight"].float())


def clip_scores(img: torch.Tensor, txt: torch.Tensor) -> torch.Tensor:
    img = img.double() / img.double().norm(dim=-1, keepdim=True)
    txt = txt.double() / txt.double().norm(dim=-1, keepdim=True)
    return 100 * (img * txt).sum(-1)
