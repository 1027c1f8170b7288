"""Prompt source of the harness (``src/dataset/dataset.py:8-41``).  The reference lists an image
directory and looks each file's prompt up in a JSON dict; the image directory is not part of the
repository, so when it is absent the prompts are taken in file order --
the hot path only consumes the prompt strings."""
from __future__ import annotations

import json
import os

import torch


def image_transform(img, size: int) -> torch.Tensor:
    """The reference's image transform (``src/experiments/base_experiment.py:79-85``: ``Resize(size)``,
    ``CenterCrop(size)``, ``ToTensor()``) restated on Pillow alone: the SHORTER side is resized to ``size`` with bilinear
    interpolation and the other to ``int(size * long / short)``, the centre ``size x size`` window is cut
    (offset ``int(round((side - size) / 2))``), and the uint8 RGB values are divided by 255 -> fp32 ``[3, size, size]``."""
    import numpy as np
    from PIL import Image
    img = img.convert("RGB")
    w, h = img.size
    if w <= h:
        nw, nh = size, int(size * h / w)
    else:
        nh, nw = size, int(size * w / h)
    if (nw, nh) != (w, h):
        img = img.resize((nw, nh), Image.BILINEAR)
    left, top = int(round((nw - size) / 2.0)), int(round((nh - size) / 2.0))
    img = img.crop((left, top, left + size, top + size))
    return torch.from_numpy(np.asarray(img, dtype=np.float32) / 255.0).permute(2, 0, 1).contiguous()


def load_image(path: str, size: int) -> torch.Tensor:
    from PIL import Image
    with Image.open(path) as im:
        return image_transform(im, size)


class PromptDataset:
    def __init__(self, image_dir: str, prompts_file: str):
        with open(prompts_file, "r") as f:
            self.prompts_json = json.load(f)
        if image_dir and os.path.isdir(image_dir):
            self.image_files = [f for f in os.listdir(image_dir) if os.path.isfile(os.path.join(image_dir, f))
                                and f in self.prompts_json]
        else:
            self.image_files = list(self.prompts_json.keys())

    def __len__(self):
        return len(self.image_files)

    def __getitem__(self, idx):
        f = self.image_files[idx]
        return {"image_file": f, "prompt": self.prompts_json[f]}

    def batches(self, batch_size: int):
        """DataLoader(batch_size, shuffle=False) equivalent."""
        for s in range(0, len(self), batch_size):
            items = [self[i] for i in range(s, min(len(self), s + batch_size))]
            yield {"image_file": [it["image_file"] for it in items], "prompt": [it["prompt"] for it in items]}
