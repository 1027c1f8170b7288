"""Images/s of CLIP scoring on libsdhip against the transformers host path, on 64 seeded uint8 images of 512x512 with
synthetic ViT-B/16 (openai/clip-vit-base-patch16 shapes) weights.  Prints one JSON line with two comparisons:
  * image side: the HIP vision tower (preprocessing + ViT + projection) against CLIPImageProcessor (PIL backend) +
    CLIPVisionModelWithProjection in fp32 on the CPU;
  * whole scorer, image-prompt pairs per second: HipClipScorer.score_pairs (tokenizer, both towers, score) against the
    ClipScoreMetric host path (processor, CLIPModel.get_image_features / get_text_features, cosine).

    timeout -k 10 900 python tools/clip_score_speed.py [--images 64] [--size 512] [--batch 32] [--threads 16]

The host path uses --threads torch threads (a GPU job gets 16 CPUs).  Both scorers tokenize with the byte-level
ClipBpeTokenizer (no checkpoint vocabulary exists offline)."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--skip-host", action="store_true")
    a = ap.parse_args()
    from sonicdiffusionbayeslab_amd.clip_score import ClipVisionConfig, HipClipVisionModel, make_synthetic_clip_vision_state_dict
    cfg = ClipVisionConfig()
    sd = make_synthetic_clip_vision_state_dict(cfg, seed=1)
    g = torch.Generator().manual_seed(0)
    imgs = torch.randint(0, 256, (a.images, 3, a.size, a.size), generator=g, dtype=torch.uint8)
    res = {"images": a.images, "size": a.size, "batch": a.batch, "model": "ViT-B/16 (synthetic weights)"}

    m = HipClipVisionModel(cfg, sd)
    dev = imgs.to("cuda")
    m.encode(dev[:a.batch])                       # plan, workspace, first launches
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for s in range(0, a.images, a.batch):
        m.encode(dev[s:s + a.batch])
    torch.cuda.synchronize()
    hip_s = time.perf_counter() - t0
    t0 = time.perf_counter()                      # with the host -> device copy of the uint8 images
    for s in range(0, a.images, a.batch):
        m.encode(imgs[s:s + a.batch])
    torch.cuda.synchronize()
    res["hip_images_per_s"] = a.images / hip_s
    res["hip_images_per_s_incl_upload"] = a.images / (time.perf_counter() - t0)

    # whole scorer: tokenizer + text tower + vision tower + score, uint8 images from the host
    from sonicdiffusionbayeslab_amd.clip import (ClipBpeTokenizer, ClipTextConfig, HipClipTextModel,
                                                 make_synthetic_clip_state_dict)
    from sonicdiffusionbayeslab_amd.clip_score import HipClipScorer
    tcfg = ClipTextConfig(hidden_size=512, num_attention_heads=8, intermediate_size=2048)
    tsd = make_synthetic_clip_state_dict(tcfg, seed=2)
    tproj = (torch.randn(cfg.projection_dim, tcfg.hidden_size, generator=g) / tcfg.hidden_size ** 0.5).to(torch.bfloat16).float()
    tok = ClipBpeTokenizer.byte_level()
    words = ["a", "photo", "of", "the", "cat", "on", "snowboard", "street", "bird", "eating", "bread", "beach", "people"]
    prompts = [" ".join(words[(i * 7 + j * 3) % len(words)] for j in range(4 + i % 9)) for i in range(a.images)]
    scorer = HipClipScorer(HipClipTextModel(tcfg, tsd, text_projection=tproj), m, tok)
    scorer.score_pairs(imgs[:a.batch], prompts[:a.batch])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for s in range(0, a.images, a.batch):
        scorer.score_pairs(imgs[s:s + a.batch], prompts[s:s + a.batch])[1].sum().item()
    res["hip_scorer_pairs_per_s"] = a.images / (time.perf_counter() - t0)

    if not a.skip_host:
        torch.set_num_threads(a.threads)
        from transformers import CLIPVisionConfig, CLIPVisionModelWithProjection
        from transformers.models.clip.image_processing_pil_clip import CLIPImageProcessorPil
        hf = CLIPVisionModelWithProjection(CLIPVisionConfig(hidden_act="quick_gelu", projection_dim=512, patch_size=16)).eval()
        hf.load_state_dict({k: v for k, v in sd.items()}, strict=False)
        proc = CLIPImageProcessorPil()
        with torch.no_grad():
            hf(pixel_values=proc(images=list(imgs[:2]), return_tensors="pt")["pixel_values"])
            t0 = time.perf_counter()
            for s in range(0, a.images, a.batch):
                pix = proc(images=list(imgs[s:s + a.batch]), return_tensors="pt")["pixel_values"]
                hf(pixel_values=pix)
            res["host_images_per_s"] = a.images / (time.perf_counter() - t0)
        from transformers import CLIPConfig, CLIPModel
        full = CLIPModel(CLIPConfig(text_config=dict(hidden_act="quick_gelu", vocab_size=tcfg.vocab_size, hidden_size=512,
                                                     num_attention_heads=8, intermediate_size=2048,
                                                     eos_token_id=tok.eos_token_id),
                                    vision_config=dict(hidden_act="quick_gelu", patch_size=16),
                                    projection_dim=cfg.projection_dim)).eval()
        full_sd = {k: v for k, v in sd.items() if k != "visual_projection.weight"}
        full_sd.update(tsd)
        full_sd["visual_projection.weight"], full_sd["text_projection.weight"] = sd["visual_projection.weight"], tproj
        full.load_state_dict(full_sd, strict=False)
        emb = lambda o: o if torch.is_tensor(o) else o.pooler_output
        with torch.no_grad():
            t0 = time.perf_counter()
            for s in range(0, a.images, a.batch):
                pix = proc(images=list(imgs[s:s + a.batch]), return_tensors="pt")["pixel_values"]
                ids = tok(prompts[s:s + a.batch]).long()
                im = emb(full.get_image_features(pixel_values=pix))
                tx = emb(full.get_text_features(input_ids=ids, attention_mask=torch.ones_like(ids)))
                (100 * torch.nn.functional.cosine_similarity(im, tx)).clamp(min=0).sum().item()
            res["host_scorer_pairs_per_s"] = a.images / (time.perf_counter() - t0)
        res["host_threads"] = a.threads
        res["speedup"] = res["hip_images_per_s"] / res["host_images_per_s"]
        res["scorer_speedup"] = res["hip_scorer_pairs_per_s"] / res["host_scorer_pairs_per_s"]
    print(json.dumps(res), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
