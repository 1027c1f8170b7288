"""CPU oracle of diffusers 0.32 ``AutoencoderTiny`` (TAESD), upstream-recall: the two halves as ``torch.nn`` modules in the
upstream layout -- an ``nn.Sequential`` named ``layers``, blocks with ``conv`` / ``skip`` / ``fuse`` -- so that
``load_state_dict(strict=True)`` of a diffusers state dict pins the key table.  Forward is fp32.

``emulate_bf16=True`` rounds to bf16 what the HIP plan stores in bf16: the weights of the 64 -> 64 convs and of the exit conv
(the entry conv runs in fp32 on fp32 weights) and every activation tensor the plan writes, i.e. each conv's output AFTER its
epilogue -- a block's third conv stays in fp32 until after the residual add and its ReLU.  Sums stay fp32 (the oracle's order
of additions is PyTorch's, not the kernel's)."""
from __future__ import annotations

import torch
import torch.nn as nn
import torch.nn.functional as F


def _r(x: torch.Tensor, on: bool) -> torch.Tensor:
    return x.to(torch.bfloat16).float() if on else x


class AutoencoderTinyBlock(nn.Module):
    def __init__(self, cin: int, cout: int):
        super().__init__()
        self.conv = nn.Sequential(nn.Conv2d(cin, cout, 3, padding=1), nn.ReLU(), nn.Conv2d(cout, cout, 3, padding=1), nn.ReLU(),
                                  nn.Conv2d(cout, cout, 3, padding=1))
        self.skip = nn.Conv2d(cin, cout, 1, bias=False) if cin != cout else nn.Identity()
        self.fuse = nn.ReLU()
        self.emulate_bf16 = False

    def forward(self, x):
        e = self.emulate_bf16
        c = self.conv
        h = _r(F.relu(F.conv2d(x, _r(c[0].weight, e), c[0].bias, padding=1)), e)
        h = _r(F.relu(F.conv2d(h, _r(c[2].weight, e), c[2].bias, padding=1)), e)
        h = F.conv2d(h, _r(c[4].weight, e), c[4].bias, padding=1)
        return _r(self.fuse(h + self.skip(x)), e)


class _Conv(nn.Conv2d):
    """A conv of ``layers`` outside the blocks.  ``round_w``: its weights are bf16 operands in the HIP plan; ``round_out``:
    its output is stored in bf16."""
    emulate_bf16 = False
    round_w = True
    round_out = True

    def forward(self, x):
        e = self.emulate_bf16
        y = F.conv2d(x, _r(self.weight, e and self.round_w), self.bias, self.stride, self.padding)
        return _r(y, e and self.round_out)


class _ReLUStore(nn.ReLU):
    """The ReLU behind the decoder's entry conv: the HIP entry kernel stores AFTER it (one rounding of relu(conv))."""
    emulate_bf16 = False

    def forward(self, x):
        return _r(F.relu(x), self.emulate_bf16)


class DecoderTiny(nn.Module):
    def __init__(self, in_channels=4, out_channels=3, num_blocks=(3, 3, 3, 1), block_out_channels=(64, 64, 64, 64)):
        super().__init__()
        entry = _Conv(in_channels, block_out_channels[0], 3, padding=1)
        entry.round_w = entry.round_out = False         # fp32 conv; the store follows the ReLU
        layers = [entry, _ReLUStore()]
        for i, nb in enumerate(num_blocks):
            c = block_out_channels[i]
            is_final = i == len(num_blocks) - 1
            for _ in range(nb):
                layers.append(AutoencoderTinyBlock(c, c))
            if not is_final:
                layers.append(nn.Upsample(scale_factor=2, mode="nearest"))
            conv_out = c if not is_final else out_channels
            last = _Conv(c, conv_out, 3, padding=1, bias=is_final)
            last.round_out = not is_final                # the exit writes fp32
            layers.append(last)
        self.layers = nn.Sequential(*layers)

    def forward(self, z):
        x = torch.tanh(z / 3) * 3
        return self.layers(x) * 2 - 1


class EncoderTiny(nn.Module):
    def __init__(self, in_channels=3, out_channels=4, num_blocks=(1, 3, 3, 3), block_out_channels=(64, 64, 64, 64)):
        super().__init__()
        layers = []
        for i, nb in enumerate(num_blocks):
            c = block_out_channels[i]
            if i == 0:
                entry = _Conv(in_channels, c, 3, padding=1)
                entry.round_w = False                    # fp32 conv, its output stored in bf16 as it is (no activation)
                layers.append(entry)
            else:
                layers.append(_Conv(c, c, 3, padding=1, stride=2, bias=False))
            for _ in range(nb):
                layers.append(AutoencoderTinyBlock(c, c))
        last = _Conv(block_out_channels[-1], out_channels, 3, padding=1)
        last.round_out = False
        layers.append(last)
        self.layers = nn.Sequential(*layers)

    def forward(self, x_pm1):
        """``x_pm1``: the image in [-1, 1] (what the pipeline's image processor hands the model)."""
        return self.layers((x_pm1 + 1) / 2)


class AutoencoderTiny(nn.Module):
    def __init__(self):
        super().__init__()
        self.encoder = EncoderTiny()
        self.decoder = DecoderTiny()

    def set_emulate_bf16(self, on: bool):
        for m in self.modules():
            if hasattr(m, "emulate_bf16"):
                m.emulate_bf16 = bool(on)
        return self

    @torch.no_grad()
    def decode(self, z, emulate_bf16: bool = False):
        """UNet latents as they are (scaling_factor 1.0) -> image in [-1, 1]."""
        self.set_emulate_bf16(emulate_bf16)
        return self.decoder(z.float())

    @torch.no_grad()
    def encode01(self, images01, emulate_bf16: bool = False):
        """Image in [0, 1] -> latents: the pipeline's ``2 x - 1`` followed by the model's ``(x + 1) / 2``."""
        self.set_emulate_bf16(emulate_bf16)
        return self.encoder(images01.float() * 2 - 1)


def build(state_dict) -> AutoencoderTiny:
    m = AutoencoderTiny()
    m.load_state_dict({k: v.float() for k, v in state_dict.items()}, strict=True)
    return m.eval()
