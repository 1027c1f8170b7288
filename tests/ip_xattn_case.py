"""Operands, float64 reference and a-priori per-element bound of ``sd_op_ip_xattn``, shared by the GPU operator test
(tests/test_ip_adapter_gpu.py) and the CPU test that the bound discriminates (tests/test_ip_adapter_cpu.py).

The bound.  The kernel normalises each row itself -- mean and centred variance in fp32 from the row, (x - mean) rstd gamma +
beta in fp32 -- and ROUNDS the normalised row to bf16 before the first product.  Per element of the normalised row: one bf16
ulp (the rounding) plus the fp32 statistics terms (mean of C terms, variance of C terms through 1 / sqrt, three
multiply-adds), carried through |A| into the scores together with the fp32 accumulation over C; through the softmax as
|dp| <= p (e^{ds + max ds} - 1); 2^-9 for the bf16 probabilities; fp32 accumulation over the 32 slots plus the residual; one
output ulp.

Two operand families.  The bound is a worst case: the ulp of the normalised row adds up LINEARLY over the channels an A row
touches and over the heads that feed an output channel, while the image branch itself grows like their square roots.

* ``dense``: every A row and every B column full, as in the UNet.  Exercises every load of the kernel, but over 320 .. 1280
  channels the worst case (a score uncertainty of ~0.25, a probability uncertainty of ~0.7) is LARGER than the branch, so on
  these operands the check sees addressing, tails, guards and finiteness, not the arithmetic.
* ``sharp``: every A row lives on ONE channel (another one per row, sample and slot, amplitude 2) and every output channel
  listens to ONE head (channel c to head c mod heads).  The same kernel code runs -- it does not know -- but the worst case
  shrinks to a few per cent of the branch, the output ulp its largest term: a wrong scale, softmax, gamma, beta or sample
  shows in most elements.  tests/test_ip_adapter_cpu.py asserts exactly that on ``PERTURBED`` below, without a GPU."""
import torch

from tests.bounds import ATOL_TINY, U32, U_BF16, ulp_bf16

T = 4
EPS = 1e-5
# (UB, rows_per_sample, C, heads)
SHAPES = [(2, 1, 1280, 8),        # one token per sample (the mid block of an 8x8 latent)
          (3, 16, 1280, 8),       # several samples inside what would be one 32-row tile
          (2, 40, 640, 8),        # tail rows
          (2, 1024, 320, 8),
          (4, 256, 640, 8),       # operands different in every sample
          (2, 40, 320, 2)]        # fewer heads: the slot groups between them get p = 0
FAMILIES = ("dense", "sharp")


def _bf(t):
    return t.to(torch.bfloat16).float()


def operands(UB, rps, C, heads, family):
    """(r [M, C], A [UB, 32, C], Bt [UB, C, 32], gamma [C], beta [C]): bf16 values as floats, gamma / beta fp32."""
    g = torch.Generator().manual_seed(1000 * UB + rps + C + heads)
    M = UB * rps
    r = _bf(torch.randn(M, C, generator=g) * (0.5 + 2.0 * torch.rand(M, 1, generator=g)) + 0.5 * torch.randn(M, 1, generator=g))
    if family == "dense":
        A = torch.randn(UB, 32, C, generator=g) * (3.0 / C ** 0.5)
        Bt = torch.randn(UB, C, 32, generator=g) * 0.5
    else:
        chan = torch.randint(0, C, (UB, 32, 1), generator=g)
        A = torch.zeros(UB, 32, C).scatter_(-1, chan, 2.0 * torch.randn(UB, 32, 1, generator=g))
        slot_head = torch.arange(32) // (32 // heads)
        Bt = torch.randn(UB, C, 32, generator=g) * 0.5 * (torch.arange(C)[:, None] % heads == slot_head[None, :]).float()
    # the layout of sd_unet_set_ip_adapter_hw: head h owns slots h * (32 / heads) .. + T, the rest are zero
    keep = torch.zeros(32)
    for h in range(heads):
        keep[h * (32 // heads): h * (32 // heads) + T] = 1.0
    A, Bt = _bf(A) * keep[None, :, None], _bf(Bt) * keep[None, None, :]
    gamma = 1.0 + 0.3 * torch.randn(C, generator=g)
    beta = 0.3 * torch.randn(C, generator=g)
    return r, A, Bt, gamma, beta


def ref_bound(r, A, Bt, gamma, beta, eps, UB, rps, C, heads, uniform=False):
    """fp64 reference [UB, rps, C], per-element bound and the image branch alone, from the operands the kernel reads.
    ``uniform`` replaces the scores by zeros (a perturbed reference for the discrimination test)."""
    x = r.double().view(UB, rps, C)
    g, b = gamma.double(), beta.double()
    mean = x.mean(-1, keepdim=True)
    c = x - mean
    var = (c * c).mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    xn = c * rstd * g + b
    # fp32 statistics from the row: the mean of C terms (any order), the centred sum of squares, 1 / sqrt
    em = (C + 1) * U32 * x.abs().mean(-1, keepdim=True)
    rho_v = (C + 5) * U32 + em * em / (var + eps)
    rho_r = 0.5 * rho_v + 4 * U32
    dxn = ulp_bf16(xn) + g.abs() * rstd * em + (c * rstd * g).abs() * (rho_r + 3 * U32) + U32 * xn.abs()
    A64 = A.double()
    S = torch.einsum("bmc,bkc->bmk", xn, A64)
    if uniform:
        S = torch.zeros_like(S)
    Smag = torch.einsum("bmc,bkc->bmk", xn.abs() + dxn, A64.abs())
    dS = torch.einsum("bmc,bkc->bmk", dxn, A64.abs()) + (C + 4) * U32 * Smag
    Sg, dg = S.view(UB, rps, 8, T), dS.view(UB, rps, 8, T)
    dg = dg + 4 * U32 * (Sg.abs() + Sg.abs().amax(-1, keepdim=True))           # the exp2 argument
    p = torch.softmax(Sg, -1)
    pe = p * (torch.exp(dg + dg.amax(-1, keepdim=True)) - 1.0) + U_BF16 * p + (T + 8) * U32 * p
    live = torch.zeros(8, dtype=torch.float64)
    live[:: 8 // heads] = 1.0                                                     # slot groups that are heads; the others: p = 0
    p, pe = (p * live[:, None]).reshape(UB, rps, 32), (pe * live[:, None]).reshape(UB, rps, 32)
    B64 = Bt.double()                                                              # [UB, C, 32]
    branch = torch.einsum("bmk,bck->bmc", p, B64)
    y = branch + x
    pa = torch.einsum("bmk,bck->bmc", p, B64.abs())
    bound = ulp_bf16(y) + torch.einsum("bmk,bck->bmc", pe, B64.abs()) + U32 * (32 + 3) * (pa + x.abs()) + ATOL_TINY
    return y, bound, branch


def perturbed(r, A, Bt, gamma, beta, eps, UB, rps, C, heads):
    """Outputs of kernels that are wrong in one way each: name -> [UB, rps, C] float64."""
    args = (eps, UB, rps, C, heads)
    y, _, branch = ref_bound(r, A, Bt, gamma, beta, *args)
    x = y - branch
    return {"no image branch": x,
            "branch x 0.5": x + 0.5 * branch,
            "branch x 0.9": x + 0.9 * branch,
            "uniform softmax": ref_bound(r, A, Bt, gamma, beta, *args, uniform=True)[0],
            "beta dropped": ref_bound(r, A, Bt, gamma, torch.zeros_like(beta), *args)[0],
            "gamma dropped": ref_bound(r, A, Bt, torch.ones_like(gamma), beta, *args)[0],
            "the next sample's operands": ref_bound(r, A.roll(1, 0), Bt.roll(1, 0), gamma, beta, *args)[0]}
