"""The tiny ImageReward of the ImageReward tests: config, a synthetic ``vocab.txt``, seeded weights, seeded images of mixed
sizes, prompts of mixed lengths, and a local model directory written from them (``ImageReward.safetensors``,
``med_config.json``, ``vision_config.json``, ``vocab.txt``).  tests/golden/make_image_reward_golden.py records transformers'
BLIP modules and BertTokenizer on it."""
from __future__ import annotations

import json
import os

import torch

# vision: 64 / 16 -> 17 tokens, three heads of 64; text: two heads of 64, encoder_width = the vision width
VISION_TINY = dict(hidden_size=192, num_hidden_layers=2, num_attention_heads=3, intermediate_size=384, image_size=64,
                   patch_size=16, layer_norm_eps=1e-6)
TEXT_TINY = dict(hidden_size=128, num_hidden_layers=2, num_attention_heads=2, intermediate_size=256, encoder_width=192,
                 max_position_embeddings=64, layer_norm_eps=1e-12, hidden_act="gelu", position_embedding_type="absolute")
WEIGHT_SEED = 909
TOL = 1.5e-2                                    # the project's tower gate (tests/test_clip_gpu.py), rel-L2 on features

IMAGE_SIZES = [(64, 64), (80, 96), (37, 53), (128, 100)]      # (H, W); two images of each, interleaved so that groups mix
IMAGE_SEEDS = [11, 12, 13, 14, 15, 16, 17, 18]
PROMPTS = [
    "A Photo of THE Cat",                       # case
    "naïve café photo",                       # accents
    "the cat's hat, red!",                      # punctuation
    "a quartz dog",                             # an unknown word
    "",                                         # [CLS] [SEP] only
    "the cat and the hat " * 10,                # longer than 35 tokens: truncated, [SEP] kept
    "running dogs jumped",                      # ## pieces
    "blue   thing\tand 123",                    # whitespace, digits
]
RANK_PROMPT = "a photo of the red cat"
RANK_IMAGES = [4, 6, 1, 5]                      # images ranked under RANK_PROMPT (mixed sizes; neighbouring rewards > 2 tol_r apart)
# win-rate pairs (real image index, generated image index, prompt index): chosen so that the oracle's reward gap exceeds
# 2 tol_r (tests/test_image_reward_cpu.py asserts it), so no decision can flip within the feature tolerance
PAIRS = [(0, 1, 0), (2, 3, 1), (4, 5, 2), (6, 7, 3), (1, 6, 6), (3, 4, 7)]


def synthetic_vocab():
    """A few hundred WordPiece entries in bert-base-uncased's layout: specials first ([PAD] = 0), then characters, ``##``
    continuations and words.  No 'q' and no 'z': a word holding one is [UNK]."""
    toks = ["[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]"] + [f"[unused{i}]" for i in range(5)]
    letters = [c for c in "abcdefghijklmnoprstuvwxy"]
    toks += list("!\"#$%&'()*+,-./:;<=>?@[\\]^_`{|}~") + list("0123456789") + letters
    toks += ["##" + c for c in letters] + ["##" + c for c in "0123456789"]
    words = ["the", "a", "of", "and", "photo", "cat", "hat", "thing", "red", "blue", "dog", "run", "jump", "naive", "cafe",
             "in", "on", "with", "big", "small", "green", "tree", "house", "car", "bird", "sky", "water", "two", "three", "man",
             "woman", "child", "old", "new", "white", "black", "12", "paint", "draw", "style"]
    toks += words
    toks += ["##s", "##ing", "##ed", "##er", "##ly", "##ning", "##es", "##ness", "##at", "##og", "##un", "##mp", "##23"]
    seen, out = set(), []
    for t in toks:
        if t not in seen:
            seen.add(t)
            out.append(t)
    return out


def tiny_config():
    from sonicdiffusionbayeslab_amd.image_reward import ImageRewardConfig
    v, t = VISION_TINY, TEXT_TINY
    return ImageRewardConfig(
        vision_hidden_size=v["hidden_size"], vision_num_hidden_layers=v["num_hidden_layers"],
        vision_num_attention_heads=v["num_attention_heads"], vision_intermediate_size=v["intermediate_size"],
        image_size=v["image_size"], patch_size=v["patch_size"], vision_layer_norm_eps=v["layer_norm_eps"],
        vocab_size=len(synthetic_vocab()), hidden_size=t["hidden_size"], num_hidden_layers=t["num_hidden_layers"],
        num_attention_heads=t["num_attention_heads"], intermediate_size=t["intermediate_size"],
        max_position_embeddings=t["max_position_embeddings"], layer_norm_eps=t["layer_norm_eps"])


def tiny_tokenizer():
    from sonicdiffusionbayeslab_amd.image_reward import BertWordPieceTokenizer
    return BertWordPieceTokenizer({t: i for i, t in enumerate(synthetic_vocab())}, max_length=tiny_config().max_text_len)


def tiny_state_dict():
    from sonicdiffusionbayeslab_amd.image_reward import make_synthetic_image_reward_state_dict
    return make_synthetic_image_reward_state_dict(tiny_config(), seed=WEIGHT_SEED)


def seeded_image(h, w, seed):
    """uint8 [3,H,W]: smooth structure plus noise, so every tap of the resize filter matters."""
    g = torch.Generator().manual_seed(seed)
    base = torch.rand(3, 1, 1, generator=g) * 255
    yy = torch.linspace(0, 1, h)[:, None]
    xx = torch.linspace(0, 1, w)[None, :]
    grad = 80 * torch.sin(6.28 * (yy * torch.rand(1, generator=g) * 3 + xx * torch.rand(1, generator=g) * 5))
    noise = torch.randint(-60, 61, (3, h, w), generator=g).float()
    return (base + grad + noise).clamp(0, 255).round().to(torch.uint8)


def tiny_images():
    """Eight images, sizes interleaved (64x64, 80x96, 37x53, 128x100, 64x64, ...): a list call has to group them."""
    return [seeded_image(*IMAGE_SIZES[i % 4], seed=s) for i, s in enumerate(IMAGE_SEEDS)]


def write_tiny_dir(d: str) -> str:
    from safetensors.torch import save_file
    os.makedirs(d, exist_ok=True)
    med = dict(TEXT_TINY, vocab_size=len(synthetic_vocab()), architectures=["BertModel"], model_type="bert",
               add_cross_attention=True, pad_token_id=0, type_vocab_size=2, attention_probs_dropout_prob=0.1,
               hidden_dropout_prob=0.1, initializer_range=0.02)
    json.dump(med, open(os.path.join(d, "med_config.json"), "w"), indent=1)
    json.dump(VISION_TINY, open(os.path.join(d, "vision_config.json"), "w"), indent=1)
    open(os.path.join(d, "vocab.txt"), "w", encoding="utf-8").write("\n".join(synthetic_vocab()) + "\n")
    save_file({k: v.contiguous() for k, v in tiny_state_dict().items()}, os.path.join(d, "ImageReward.safetensors"))
    return d


def tol_r(cfg, sd, f_ref: torch.Tensor) -> torch.Tensor:
    """Per-sample reward tolerance implied by the feature gate: |w . (f - f_ref)| <= ||w|| TOL ||f_ref||, over std."""
    from sonicdiffusionbayeslab_amd.image_reward import fold_reward_head
    w, _ = fold_reward_head(sd)
    return TOL * f_ref.double().norm(dim=-1) * float(w.norm()) / cfg.reward_std


def oracle_decisions(cfg, sd, tok, images):
    """Per pair of PAIRS: does the generated image win (reward_real <= reward_gen) under the fp32 oracle?"""
    from tests import image_reward_oracle as O
    real = O.score(sd, cfg, tok, [PROMPTS[p] for _, _, p in PAIRS], [images[r] for r, _, _ in PAIRS])
    gen = O.score(sd, cfg, tok, [PROMPTS[p] for _, _, p in PAIRS], [images[g] for _, g, _ in PAIRS])
    return (real <= gen).tolist()
