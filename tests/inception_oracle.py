"""fp32 oracle of the FID Inception-v3 ("pt_inception-2015-12-05": torch-fidelity's FeatureExtractorInceptionV3, the
network behind torchmetrics' FrechetInceptionDistance) in plain ``torch.nn.functional`` on the CPU.  UNPINNED: neither
torch-fidelity nor torchvision is available offline, so this restates the architecture from its published description; it
takes the same state dict as ``sonicdiffusionbayeslab_amd.fid``.

``round_bf16=True`` emulates the storage precision of the HIP network: every conv's input, its folded weight and its output
are rounded to bf16 (pools and means then run on those rounded tensors in fp32).  It is the reference-against-reference run
from which the tests derive their gates.
"""
import torch
import torch.nn.functional as F

BN_EPS = 1e-3
SIDE = 299
TAPS = (64, 192, 768, 2048)


def tf1_resize(x, side=SIDE):
    """uint8 / float ``[B,3,H,W]`` -> fp32 ``[B,3,side,side]``: TensorFlow-1 legacy bilinear (no half-pixel offset:
    ``src = dst * (in / out)``, ``lo = floor(src)``, ``hi = min(lo + 1, in - 1)``, ``d = src - lo``), lerp along x first,
    then along y, every step one fp32 operation."""
    x = x.float()
    _, _, h, w = x.shape

    def taps(n_in):
        scale = torch.tensor(float(n_in), dtype=torch.float32) / torch.tensor(float(side), dtype=torch.float32)
        src = torch.arange(side, dtype=torch.float32) * scale
        lo = src.floor().clamp(max=n_in - 1)
        hi = (lo + 1).clamp(max=n_in - 1)
        return lo.long(), hi.long(), src - lo

    y0, y1, dy = taps(h)
    x0, x1, dx = taps(w)
    dx = dx.view(1, 1, 1, -1)
    dy = dy.view(1, 1, -1, 1)
    rows0, rows1 = x[:, :, y0, :], x[:, :, y1, :]
    top = rows0[..., x0] + (rows0[..., x1] - rows0[..., x0]) * dx
    bot = rows1[..., x0] + (rows1[..., x1] - rows1[..., x0]) * dx
    return top + (bot - top) * dy


def preprocess(images):
    return (tf1_resize(images) - 128.0) / 128.0


def _r(t, on):
    return t.bfloat16().float() if on else t


class Oracle:
    def __init__(self, sd, round_bf16=False):
        self.sd, self.rb = sd, round_bf16
        self.shapes = {}                    # name -> output shape of every conv block and block output (layer-table test)

    def conv(self, name, x, stride=1, padding=0):
        sd = self.sd
        w = sd[f"{name}.conv.weight"].double()
        scale = sd[f"{name}.bn.weight"].double() / torch.sqrt(sd[f"{name}.bn.running_var"].double() + BN_EPS)
        wf = (w * scale.view(-1, 1, 1, 1)).float()
        bf = (sd[f"{name}.bn.bias"].double() - sd[f"{name}.bn.running_mean"].double() * scale).float()
        y = F.relu(F.conv2d(_r(x, self.rb), _r(wf, self.rb), bf, stride=stride, padding=padding))
        y = _r(y, self.rb)
        self.shapes[name] = tuple(y.shape)
        return y

    def avg(self, x):
        return _r(F.avg_pool2d(x, 3, stride=1, padding=1, count_include_pad=False), self.rb)

    def block_a(self, p, x):
        c = self.conv
        b1 = c(p + "branch1x1", x)
        b5 = c(p + "branch5x5_2", c(p + "branch5x5_1", x), padding=2)
        b3 = c(p + "branch3x3dbl_3", c(p + "branch3x3dbl_2", c(p + "branch3x3dbl_1", x), padding=1), padding=1)
        bp = c(p + "branch_pool", self.avg(x))
        return torch.cat([b1, b5, b3, bp], 1)

    def block_b(self, p, x):
        c = self.conv
        b3 = c(p + "branch3x3", x, stride=2)
        bd = c(p + "branch3x3dbl_3", c(p + "branch3x3dbl_2", c(p + "branch3x3dbl_1", x), padding=1), stride=2)
        return torch.cat([b3, bd, F.max_pool2d(x, 3, stride=2)], 1)

    def block_c(self, p, x):
        c = self.conv
        b1 = c(p + "branch1x1", x)
        b7 = c(p + "branch7x7_3", c(p + "branch7x7_2", c(p + "branch7x7_1", x), padding=(0, 3)), padding=(3, 0))
        bd = c(p + "branch7x7dbl_1", x)
        bd = c(p + "branch7x7dbl_2", bd, padding=(3, 0))
        bd = c(p + "branch7x7dbl_3", bd, padding=(0, 3))
        bd = c(p + "branch7x7dbl_4", bd, padding=(3, 0))
        bd = c(p + "branch7x7dbl_5", bd, padding=(0, 3))
        bp = c(p + "branch_pool", self.avg(x))
        return torch.cat([b1, b7, bd, bp], 1)

    def block_d(self, p, x):
        c = self.conv
        b3 = c(p + "branch3x3_2", c(p + "branch3x3_1", x), stride=2)
        b7 = c(p + "branch7x7x3_1", x)
        b7 = c(p + "branch7x7x3_2", b7, padding=(0, 3))
        b7 = c(p + "branch7x7x3_3", b7, padding=(3, 0))
        b7 = c(p + "branch7x7x3_4", b7, stride=2)
        return torch.cat([b3, b7, F.max_pool2d(x, 3, stride=2)], 1)

    def block_e(self, p, x, max_pool):
        c = self.conv
        b1 = c(p + "branch1x1", x)
        b3 = c(p + "branch3x3_1", x)
        b3 = torch.cat([c(p + "branch3x3_2a", b3, padding=(0, 1)), c(p + "branch3x3_2b", b3, padding=(1, 0))], 1)
        bd = c(p + "branch3x3dbl_2", c(p + "branch3x3dbl_1", x), padding=1)
        bd = torch.cat([c(p + "branch3x3dbl_3a", bd, padding=(0, 1)), c(p + "branch3x3dbl_3b", bd, padding=(1, 0))], 1)
        pooled = F.max_pool2d(x, 3, stride=1, padding=1) if max_pool else self.avg(x)
        bp = c(p + "branch_pool", pooled)
        return torch.cat([b1, b3, bd, bp], 1)

    def forward(self, images, upto=2048):
        """``{tap: fp32 [B, tap]}`` for every tap <= ``upto``."""
        assert upto in TAPS
        out = {}
        c = self.conv
        x = preprocess(images)
        x = c("Conv2d_1a_3x3", x, stride=2)
        x = c("Conv2d_2a_3x3", x)
        x = c("Conv2d_2b_3x3", x, padding=1)
        x = F.max_pool2d(x, 3, stride=2)
        out[64] = x.mean((2, 3))
        if upto == 64:
            return out
        x = c("Conv2d_3b_1x1", x)
        x = c("Conv2d_4a_3x3", x)
        x = F.max_pool2d(x, 3, stride=2)
        out[192] = x.mean((2, 3))
        if upto == 192:
            return out
        for name in ("Mixed_5b", "Mixed_5c", "Mixed_5d"):
            x = self.block_a(name + ".", x)
            self.shapes[name] = tuple(x.shape)
        x = self.block_b("Mixed_6a.", x)
        self.shapes["Mixed_6a"] = tuple(x.shape)
        for name in ("Mixed_6b", "Mixed_6c", "Mixed_6d", "Mixed_6e"):
            x = self.block_c(name + ".", x)
            self.shapes[name] = tuple(x.shape)
        out[768] = x.mean((2, 3))
        if upto == 768:
            return out
        x = self.block_d("Mixed_7a.", x)
        self.shapes["Mixed_7a"] = tuple(x.shape)
        x = self.block_e("Mixed_7b.", x, False)
        self.shapes["Mixed_7b"] = tuple(x.shape)
        x = self.block_e("Mixed_7c.", x, True)
        self.shapes["Mixed_7c"] = tuple(x.shape)
        out[2048] = x.mean((2, 3))
        return out


@torch.no_grad()
def inception_features(sd, images, upto=2048, round_bf16=False):
    return Oracle(sd, round_bf16).forward(images, upto)
