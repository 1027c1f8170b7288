"""Record tests/golden/image_reward_golden.json: the tiny ImageReward (tests/image_reward_util.py) run through a THIRD-PARTY
implementation, so that tests/image_reward_oracle.py is pinned to something other than itself (as make_clip_golden.py does).

* ids / mask: transformers ``BertTokenizer`` over the synthetic vocab.txt, ``padding='max_length', truncation=True,
  max_length=35`` (upstream ImageReward's call).
* features: the tiny weights loaded, through the key map below, into transformers' ``BlipVisionModel`` (its
  ``last_hidden_state`` is ``post_layernorm`` over all rows; its patch conv has a bias) and ``BlipTextModel`` (word + position
  + LayerNorm embeddings) driven with ``attention_mask``, ``encoder_hidden_states`` and ``is_decoder=False``.
* rewards: ``torch.nn.Linear`` x 5 over the features, then (r - mean) / std.

Preprocessing is not part of this golden (the pixel values come from tests/clip_vision_oracle.pil_crop, which
make_clip_score_golden.py pins against CLIPImageProcessor).  Run from the repository root:
``python tests/golden/make_image_reward_golden.py``.  If a module of the installed transformers cannot be driven this way the
script says which one and stops.
"""
import json
import os
import sys
import tempfile

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
from tests import image_reward_oracle as O            # noqa: E402
from tests import image_reward_util as U              # noqa: E402


def vision_key(k: str) -> str:
    k = k[len("blip.visual_encoder."):]
    for a, b in (("cls_token", "embeddings.class_embedding"), ("pos_embed", "embeddings.position_embedding"),
                 ("patch_embed.proj.", "embeddings.patch_embedding."), ("blocks.", "encoder.layers."), (".attn.qkv.", ".self_attn.qkv."),
                 (".attn.proj.", ".self_attn.projection."), (".norm1.", ".layer_norm1."), (".norm2.", ".layer_norm2.")):
        k = k.replace(a, b)
    return "post_layernorm." + k[len("norm."):] if k.startswith("norm.") else k


@torch.no_grad()
def main():
    import transformers
    from transformers import BertTokenizer, BlipTextConfig, BlipTextModel, BlipVisionConfig, BlipVisionModel
    cfg, sd, images = U.tiny_config(), U.tiny_state_dict(), U.tiny_images()
    d = U.write_tiny_dir(tempfile.mkdtemp())
    enc = BertTokenizer(os.path.join(d, "vocab.txt"))(U.PROMPTS, padding="max_length", truncation=True, max_length=cfg.max_text_len,
                                                      return_tensors="pt")
    ids, mask = enc["input_ids"], enc["attention_mask"]

    try:
        vm = BlipVisionModel(BlipVisionConfig(
            hidden_size=cfg.vision_hidden_size, intermediate_size=cfg.vision_intermediate_size,
            num_hidden_layers=cfg.vision_num_hidden_layers, num_attention_heads=cfg.vision_num_attention_heads,
            image_size=cfg.image_size, patch_size=cfg.patch_size, layer_norm_eps=cfg.vision_layer_norm_eps, hidden_act="gelu",
            attention_dropout=0.0)).eval()
        vm.load_state_dict({vision_key(k): v for k, v in sd.items() if k.startswith("blip.visual_encoder.")}, strict=True)
        tokens = vm(pixel_values=O.preprocess(images, cfg)).last_hidden_state
    except Exception as e:
        raise SystemExit(f"BlipVisionModel of transformers {transformers.__version__} cannot be driven: {e!r}")
    try:
        tm = BlipTextModel(BlipTextConfig(
            vocab_size=cfg.vocab_size, hidden_size=cfg.hidden_size, encoder_hidden_size=cfg.vision_hidden_size,
            intermediate_size=cfg.intermediate_size, num_hidden_layers=cfg.num_hidden_layers,
            num_attention_heads=cfg.num_attention_heads, max_position_embeddings=cfg.max_position_embeddings,
            layer_norm_eps=cfg.layer_norm_eps, hidden_act="gelu", hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0,
            bos_token_id=None, pad_token_id=0, eos_token_id=None, sep_token_id=None), add_pooling_layer=False).eval()
        tm.load_state_dict({k[len("blip.text_encoder."):]: v for k, v in sd.items() if k.startswith("blip.text_encoder.")}, strict=True)
        feats = tm(input_ids=ids, attention_mask=mask, encoder_hidden_states=tokens, is_decoder=False).last_hidden_state[:, 0]
    except Exception as e:
        raise SystemExit(f"BlipTextModel of transformers {transformers.__version__} cannot be driven: {e!r}")

    x = feats
    fan = cfg.hidden_size
    for k, dim in zip((0, 2, 4, 6, 7), (1024, 128, 64, 16, 1)):
        lin = torch.nn.Linear(fan, dim)
        lin.weight.copy_(sd[f"mlp.layers.{k}.weight"]); lin.bias.copy_(sd[f"mlp.layers.{k}.bias"])
        x, fan = lin(x), dim
    rewards = (x[:, 0] - cfg.reward_mean) / cfg.reward_std

    out = {"transformers": transformers.__version__, "prompts": U.PROMPTS, "input_ids": ids.tolist(), "attention_mask": mask.tolist(),
           "features": [[round(float(v), 7) for v in row] for row in feats.tolist()], "rewards": rewards.tolist()}
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "image_reward_golden.json")
    json.dump(out, open(path, "w"))
    print(path, os.path.getsize(path), "bytes")
    of = O.features_from_ids(sd, cfg, ids.int(), mask.int(), images)
    print("oracle vs golden features rel-L2", float((of - feats).norm() / feats.norm()),
          "rewards", float((O.reward_head(sd, cfg, of) - rewards).abs().max()))


if __name__ == "__main__":
    main()
