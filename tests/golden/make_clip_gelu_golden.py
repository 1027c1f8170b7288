"""Writes tests/golden/clip_gelu_golden.json from the transformers build in this image (third-party library, NOT the
reference): what ``make_clip_golden.py`` does for the SD-1.5 text tower, for the Stable Diffusion 2.x one --
``CLIPTextModel(hidden_act="gelu")`` (the exact, erf GELU of the OpenCLIP text tower) on ids that
``transformers.CLIPTokenizer(pad_token="!")`` produces from the synthetic vocabulary of tests/util.py: SD 2.x pads with
``!``, not with ``<|endoftext|>``.  The tiny model of clip_golden.json with the weights of
``tests/sd2_oracle.py::gelu_clip_state_dict`` (which says why they differ).  Pins ``ClipBpeTokenizer``'s pad token,
``tests/sd2_oracle.py::clip_text_forward_act`` and, through it, the library's gelu text tower.
Run from the repo root: ``python tests/golden/make_clip_gelu_golden.py``."""
import json
import os
import sys
import tempfile

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from tests.sd2_oracle import gelu_clip_state_dict  # noqa: E402
from tests.util import CLIP_TEXTS, CLIP_TINY, synthetic_clip_vocab  # noqa: E402

PAD_TOKEN = "!"


def main():
    import transformers
    from transformers import CLIPTextConfig, CLIPTextModel, CLIPTokenizer
    vocab, merges = synthetic_clip_vocab()
    L = CLIP_TINY["max_position_embeddings"]
    with tempfile.TemporaryDirectory() as d:
        json.dump(vocab, open(os.path.join(d, "vocab.json"), "w"))
        open(os.path.join(d, "merges.txt"), "w").write("#version: 0.2\n" + "\n".join(f"{a} {b}" for a, b in merges) + "\n")
        tk = CLIPTokenizer(os.path.join(d, "vocab.json"), os.path.join(d, "merges.txt"), pad_token=PAD_TOKEN)
        ids = [tk(t, padding="max_length", max_length=L, truncation=True).input_ids for t in CLIP_TEXTS]
    assert tk.pad_token_id == vocab[PAD_TOKEN] != vocab["<|endoftext|>"]
    assert any(row[-1] == vocab[PAD_TOKEN] for row in ids)              # the pad token really occurs
    _, sd = gelu_clip_state_dict()
    tcfg = CLIPTextConfig(hidden_act="gelu", bos_token_id=vocab["<|startoftext|>"], eos_token_id=vocab["<|endoftext|>"],
                          pad_token_id=vocab[PAD_TOKEN], **CLIP_TINY)
    m = CLIPTextModel(tcfg).eval()
    own = m.state_dict()
    prefixed = any(k.startswith("text_model.") for k in own)
    missing = m.load_state_dict({(k if prefixed else k[len("text_model."):]): v for k, v in sd.items()}, strict=False)
    assert not [k for k in missing.missing_keys if "position_ids" not in k], missing
    with torch.no_grad():
        out = m(torch.tensor(ids)).last_hidden_state
    res = {"transformers_version": transformers.__version__, "texts": CLIP_TEXTS, "pad_token": PAD_TOKEN, "hidden_act": "gelu",
           "input_ids": ids, "weights": "tests.sd2_oracle.gelu_clip_state_dict()",
           "last_hidden_state": [[[round(float(v), 6) for v in row] for row in b] for b in out]}
    path = os.path.join(ROOT, "tests", "golden", "clip_gelu_golden.json")
    json.dump(res, open(path, "w"))
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
