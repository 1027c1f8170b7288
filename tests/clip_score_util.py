"""The tiny CLIPModel of the CLIP-score tests: configs, seeded weights, seeded images and prompts, and a local checkpoint
directory written from them (config.json, model.safetensors, vocab.json / merges.txt, tokenizer and preprocessor configs)
that both ClipScoreMetric backends load.  tests/golden/make_clip_score_golden.py records transformers on it."""
from __future__ import annotations

import json
import os

import torch

from tests.util import CLIP_TINY, synthetic_clip_vocab

# vision tower: head dim 64 (two heads of a 128-wide stream), 224 / 16 -> 197 tokens; text tower: tests/util.CLIP_TINY
VISION_TINY = dict(hidden_size=128, num_hidden_layers=2, num_attention_heads=2, intermediate_size=256, image_size=224,
                   patch_size=16, projection_dim=64)
PROJECTION_DIM = 64
IMAGE_SIZES = [(224, 224), (256, 256), (200, 300), (37, 53)]      # (H, W); two images of each
PROMPTS = ["A photo of the cat", "the thing and the hat", "naive cafe 123 photo", "", "x" * 40, "photo of of the",
           "a cat", "the  CAT and\tthe hat's thing!!"]
TEXT_SEED, VISION_SEED, PROJ_SEED, IMAGE_SEED = 777, 555, 333, 1234


def tiny_configs():
    from sonicdiffusionbayeslab_amd.clip import ClipTextConfig
    from sonicdiffusionbayeslab_amd.clip_score import ClipVisionConfig
    return ClipTextConfig(**CLIP_TINY), ClipVisionConfig(**VISION_TINY)


def tiny_state_dict():
    """CLIPModel state_dict names: text_model.*, vision_model.*, text_projection / visual_projection, logit_scale."""
    from sonicdiffusionbayeslab_amd.clip import make_synthetic_clip_state_dict
    from sonicdiffusionbayeslab_amd.clip_score import make_synthetic_clip_vision_state_dict
    tcfg, vcfg = tiny_configs()
    sd = dict(make_synthetic_clip_state_dict(tcfg, seed=TEXT_SEED))
    sd.update(make_synthetic_clip_vision_state_dict(vcfg, seed=VISION_SEED))
    g = torch.Generator().manual_seed(PROJ_SEED)
    sd["text_projection.weight"] = (torch.randn(PROJECTION_DIM, tcfg.hidden_size, generator=g) / tcfg.hidden_size ** 0.5
                                    ).to(torch.bfloat16).float()
    sd["logit_scale"] = torch.tensor(2.6592)
    return sd


def tiny_images():
    """Seeded uint8 [3,H,W] images: smooth structure plus noise, so the resize filter's every tap matters."""
    g = torch.Generator().manual_seed(IMAGE_SEED)
    out = []
    for h, w in IMAGE_SIZES:
        for _ in range(2):
            base = torch.rand(3, 1, 1, generator=g) * 255
            yy = torch.linspace(0, 1, h)[:, None]
            xx = torch.linspace(0, 1, w)[None, :]
            grad = 80 * torch.sin(6.28 * (yy * torch.rand(1, generator=g) * 3 + xx * torch.rand(1, generator=g) * 5))
            noise = torch.randint(-60, 61, (3, h, w), generator=g).float()
            out.append((base + grad + noise).clamp(0, 255).round().to(torch.uint8))
    return out


def write_tiny_clip_dir(d: str) -> str:
    from safetensors.torch import save_file
    tcfg, vcfg = tiny_configs()
    vocab, merges = synthetic_clip_vocab()
    text_config = dict(CLIP_TINY, hidden_act="quick_gelu", layer_norm_eps=1e-5, bos_token_id=vocab["<|startoftext|>"],
                       eos_token_id=vocab["<|endoftext|>"], pad_token_id=vocab["<|endoftext|>"],
                       projection_dim=PROJECTION_DIM)
    vision_config = {k: v for k, v in VISION_TINY.items() if k != "projection_dim"}
    vision_config.update(hidden_act="quick_gelu", layer_norm_eps=1e-5, num_channels=3, projection_dim=PROJECTION_DIM)
    cfg = {"architectures": ["CLIPModel"], "model_type": "clip", "projection_dim": PROJECTION_DIM,
           "logit_scale_init_value": 2.6592, "text_config": text_config, "vision_config": vision_config}
    os.makedirs(d, exist_ok=True)
    json.dump(cfg, open(os.path.join(d, "config.json"), "w"), indent=1)
    save_file({k: v.contiguous() for k, v in tiny_state_dict().items()}, os.path.join(d, "model.safetensors"))
    json.dump(vocab, open(os.path.join(d, "vocab.json"), "w"))
    open(os.path.join(d, "merges.txt"), "w").write("#version: 0.2\n" + "\n".join(f"{a} {b}" for a, b in merges) + "\n")
    json.dump({"tokenizer_class": "CLIPTokenizer", "model_max_length": CLIP_TINY["max_position_embeddings"],
               "bos_token": "<|startoftext|>", "eos_token": "<|endoftext|>", "pad_token": "<|endoftext|>",
               "unk_token": "<|endoftext|>"}, open(os.path.join(d, "tokenizer_config.json"), "w"))
    json.dump({"image_processor_type": "CLIPImageProcessor", "processor_class": "CLIPProcessor", "do_resize": True,
               "size": {"shortest_edge": 224}, "resample": 3, "do_center_crop": True,
               "crop_size": {"height": 224, "width": 224}, "do_rescale": True, "rescale_factor": 1 / 255,
               "do_normalize": True, "image_mean": [0.48145466, 0.4578275, 0.40821073],
               "image_std": [0.26862954, 0.26130258, 0.27577711], "do_convert_rgb": True},
              open(os.path.join(d, "preprocessor_config.json"), "w"))
    return d
