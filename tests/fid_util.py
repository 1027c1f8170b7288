"""Seeded stand-ins for the FID tests: the layer table of the FID Inception-v3 (written out here, independent of the library
and of tests/inception_oracle.py), a random state dict over it, and seeded uint8 images."""
import torch


def _a(p, cin, pf):
    return [(p + "branch1x1", 64, cin, 1, 1), (p + "branch5x5_1", 48, cin, 1, 1), (p + "branch5x5_2", 64, 48, 5, 5),
            (p + "branch3x3dbl_1", 64, cin, 1, 1), (p + "branch3x3dbl_2", 96, 64, 3, 3), (p + "branch3x3dbl_3", 96, 96, 3, 3),
            (p + "branch_pool", pf, cin, 1, 1)]


def _c(p, c7):
    return [(p + "branch1x1", 192, 768, 1, 1), (p + "branch7x7_1", c7, 768, 1, 1), (p + "branch7x7_2", c7, c7, 1, 7),
            (p + "branch7x7_3", 192, c7, 7, 1), (p + "branch7x7dbl_1", c7, 768, 1, 1), (p + "branch7x7dbl_2", c7, c7, 7, 1),
            (p + "branch7x7dbl_3", c7, c7, 1, 7), (p + "branch7x7dbl_4", c7, c7, 7, 1), (p + "branch7x7dbl_5", 192, c7, 1, 7),
            (p + "branch_pool", 192, 768, 1, 1)]


def _e(p, cin):
    return [(p + "branch1x1", 320, cin, 1, 1), (p + "branch3x3_1", 384, cin, 1, 1), (p + "branch3x3_2a", 384, 384, 1, 3),
            (p + "branch3x3_2b", 384, 384, 3, 1), (p + "branch3x3dbl_1", 448, cin, 1, 1), (p + "branch3x3dbl_2", 384, 448, 3, 3),
            (p + "branch3x3dbl_3a", 384, 384, 1, 3), (p + "branch3x3dbl_3b", 384, 384, 3, 1), (p + "branch_pool", 192, cin, 1, 1)]


def layer_table():
    """``[(module, Cout, Cin, kh, kw)]`` of the 94 conv blocks in forward order."""
    t = [("Conv2d_1a_3x3", 32, 3, 3, 3), ("Conv2d_2a_3x3", 32, 32, 3, 3), ("Conv2d_2b_3x3", 64, 32, 3, 3),
         ("Conv2d_3b_1x1", 80, 64, 1, 1), ("Conv2d_4a_3x3", 192, 80, 3, 3)]
    t += _a("Mixed_5b.", 192, 32) + _a("Mixed_5c.", 256, 64) + _a("Mixed_5d.", 288, 64)
    p = "Mixed_6a."
    t += [(p + "branch3x3", 384, 288, 3, 3), (p + "branch3x3dbl_1", 64, 288, 1, 1), (p + "branch3x3dbl_2", 96, 64, 3, 3),
          (p + "branch3x3dbl_3", 96, 96, 3, 3)]
    t += _c("Mixed_6b.", 128) + _c("Mixed_6c.", 160) + _c("Mixed_6d.", 160) + _c("Mixed_6e.", 192)
    p = "Mixed_7a."
    t += [(p + "branch3x3_1", 192, 768, 1, 1), (p + "branch3x3_2", 320, 192, 3, 3), (p + "branch7x7x3_1", 192, 768, 1, 1),
          (p + "branch7x7x3_2", 192, 192, 1, 7), (p + "branch7x7x3_3", 192, 192, 7, 1), (p + "branch7x7x3_4", 192, 192, 3, 3)]
    t += _e("Mixed_7b.", 1280) + _e("Mixed_7c.", 2048)
    return t


def random_state_dict(seed=0):
    """He-scaled conv weights; BatchNorm scale / variance near 1 and shift / mean near 0, each with spread, so that the
    activations neither die nor blow up through Mixed_7c.  Also carries the keys a real checkpoint has and the loader must
    ignore (``fc.*``, ``num_batches_tracked``)."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for name, cout, cin, kh, kw in layer_table():
        sd[f"{name}.conv.weight"] = torch.randn(cout, cin, kh, kw, generator=g) * (2.0 / (cin * kh * kw)) ** 0.5
        sd[f"{name}.bn.weight"] = 0.8 + 0.4 * torch.rand(cout, generator=g)
        sd[f"{name}.bn.bias"] = 0.1 * torch.randn(cout, generator=g)
        sd[f"{name}.bn.running_mean"] = 0.1 * torch.randn(cout, generator=g)
        sd[f"{name}.bn.running_var"] = 0.7 + 0.6 * torch.rand(cout, generator=g)
        sd[f"{name}.bn.num_batches_tracked"] = torch.tensor(1)
    sd["fc.weight"] = torch.zeros(1008, 2048)
    sd["fc.bias"] = torch.zeros(1008)
    return sd


def seeded_images(n, h, w, seed=0):
    """uint8 ``[n,3,h,w]``: 16-pixel colour blocks plus per-pixel noise (structure at two scales)."""
    g = torch.Generator().manual_seed(seed)
    low = torch.randint(0, 256, (n, 3, (h + 15) // 16, (w + 15) // 16), generator=g)
    img = low.repeat_interleave(16, 2).repeat_interleave(16, 3)[:, :, :h, :w]
    img = img + torch.randint(-24, 25, (n, 3, h, w), generator=g)
    return img.clamp(0, 255).to(torch.uint8)


def noisy_copies(images, seed=1, gain=0.85, noise=20):
    """The "generated" side of the metric tests: the real images times a gain plus uniform noise."""
    g = torch.Generator().manual_seed(seed)
    x = images.float() * gain + torch.randint(-noise, noise + 1, images.shape, generator=g).float()
    return x.clamp(0, 255).to(torch.uint8)


METRIC_N, METRIC_HW = 24, (96, 80)


def metric_images():
    """The 24 "real" and 24 "generated" images of the end-to-end metric tests (tests/golden/fid_golden.npz holds the fp32
    oracle's features of exactly these, real first)."""
    real = seeded_images(METRIC_N, *METRIC_HW, seed=7)
    return real, noisy_copies(real)
