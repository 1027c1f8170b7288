"""Writes tests/golden/vit_hd64_quick_gelu.safetensors: the image embeddings that ``HipClipVisionModel`` gives on a GPU for
the tiny head-dim-64 / quick_gelu vision tower of tests/clip_score_util.py (seeded weights) on its seeded uint8 images --
each image alone, and the two 224 x 224 ones as one batch.  The committed file was recorded on the commit BEFORE the tower
learned head dim 80 and exact GELU; tests/test_ip_adapter_gpu.py compares the present build with it bit for bit, so
re-record it only when the head-dim-64 tower's arithmetic is changed on purpose.  The metadata carries a SHA-256 of the
weights and images, so a drift of the seeded generators is told apart from a drift of the tower.  Run from the repo root:
``python tests/golden/make_vit_hd64_golden.py [output path]``."""
import hashlib
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from tests.clip_score_util import tiny_configs, tiny_images, tiny_state_dict  # noqa: E402

NAME = "vit_hd64_quick_gelu.safetensors"


def inputs():
    """(vision config, vision weights, images, SHA-256 of weights and images)."""
    _, vcfg = tiny_configs()
    sd = {k: v for k, v in tiny_state_dict().items() if k.startswith("vision_model.") or k == "visual_projection.weight"}
    images = tiny_images()
    h = hashlib.sha256()
    for k in sorted(sd):
        h.update(k.encode())
        h.update(sd[k].contiguous().numpy().tobytes())
    for im in images:
        h.update(im.contiguous().numpy().tobytes())
    return vcfg, sd, images, h.hexdigest()


def embed(vcfg, sd, images):
    """Each image alone, then the first two (same size) as one batch."""
    from sonicdiffusionbayeslab_amd.clip_score import HipClipVisionModel
    net = HipClipVisionModel(vcfg, sd)
    single = torch.cat([net(im[None].cuda()) for im in images]).float().cpu()
    pair = net(torch.stack(images[:2]).cuda()).float().cpu()
    return single, pair


def main():
    from safetensors.torch import save_file
    vcfg, sd, images, digest = inputs()
    single, pair = embed(vcfg, sd, images)
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", NAME)
    save_file({"image_embeds": single.contiguous(), "pair_embeds": pair.contiguous()}, path, metadata={"inputs_sha256": digest})
    print("wrote", path, os.path.getsize(path), "bytes; inputs", digest, "; embeds", tuple(single.shape), "norm", single.norm().item())


if __name__ == "__main__":
    main()
