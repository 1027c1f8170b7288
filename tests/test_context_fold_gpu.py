"""The builders of the prompt-side operands of cross-attention on their own: xattn_expand / transpose_bf16 / retile32
(csrc/small.hip) and the two launchers sd_unet_set_context_hw and sd_unet_set_ip_adapter_hw run per layer
(sd_launch_xattn_fold / sd_launch_ip_fold, csrc/unet.hip).  A whole-UNet forward at rel-L2 2e-2 cannot see an error confined to
one head's last key, to the pad slots, to the rounding of scale * K, to c1 of one slot or to one 32-column slice of one sample.

Every operand and output lives between guard bands (tests/bounds.py), outputs are pre-filled with NaN, and check_guards()
follows every launch.  Pure data movement is compared as integers.  The arithmetic stages are checked one by one from the
kernel's own stored intermediates, in fp64 from the bits the kernel reads, against a-priori bounds of tests/bounds.py.

What the three scratch slabs hold after sd_op_xattn_fold (counted from 0) is part of what these tests document: slab 0 = B^T
[UB * NP][C] in natural slot order (the second GEMM overwrote the K expansion there), slab 1 = the V expansion, slab 2 = the
permuted transpose of B^T before its re-tiling (tiled form; not written in the plain form).  After sd_op_ip_fold: the K
expansion, the V expansion (times the adapter scale), B^T [UB * 32][C].

The last section runs whole model handles after the workspace was filled with zeros, with 0xFF bytes and with NaN: what a
forward computes must not depend on what the workspace held before set_context."""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from sonicdiffusionbayeslab_amd import _lib
from tests.bounds import (U32, assert_elementwise, check_guards, forget_guards, gemm_ref, guarded, guarded_input, linear_bound,
                          ln_fold_ref_bound, xattn_elementwise, xattn_norm2_elementwise)
from tests.util import rel_l2

BF = torch.bfloat16


def stream():
    return _lib.current_stream()


def P(t):
    return t.data_ptr()


def bits(t):
    """bf16 / fp32 values as integers: comparisons that must hold bit for bit (and see -0 and NaN payloads)."""
    t = t.detach().cpu().contiguous()
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def f32(v):
    """v rounded to fp32, as a Python float (what a C float argument holds)."""
    return float(torch.tensor(v, dtype=torch.float32))


def rsqrt_f32(d):
    """1.0f / sqrtf((float)d) as the host computes it: two correctly rounded fp32 operations."""
    return float(torch.ones((), dtype=torch.float32) / torch.sqrt(torch.tensor(float(d), dtype=torch.float32)))


def perm16(r):
    """Bits 2 and 3 of the slot swapped inside every group of 16 (the only place the tests of the builders state the
    permutation; tests/test_context_fold_cpu.py checks on the host that it is an involution)."""
    return (r & ~12) | ((r & 4) << 1) | ((r & 8) >> 1)


def retile32_ref(src, B, R, K, RT):
    """[B][R][K] -> [B][R / RT][K / 32][RT][32]"""
    return src.reshape(B, R // RT, RT, K // 32, 32).permute(0, 1, 3, 2, 4).contiguous()


def untile32(t, B, R, K, RT):
    """The inverse of retile32_ref: -> [B][R][K]"""
    return t.reshape(B, R // RT, K // 32, RT, 32).permute(0, 1, 3, 2, 4).reshape(B, R, K).contiguous()


def random_bits(shape, seed):
    """bf16 tensors of arbitrary bit patterns (NaN payloads, infinities, -0 and subnormals included)."""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-32768, 32768, shape, generator=g, dtype=torch.int32).to(torch.int16).view(BF)


@pytest.fixture(autouse=True)
def _forget():
    yield
    torch.cuda.synchronize()
    forget_guards()


# ---- a. pure data movement, bit for bit ------------------------------------------------------------------------------------

def make_kv(B, L, C, seed, scale=1.0, bos=40.0):
    """Projected prompt rows [B * L][K | V] as bf16: noise, key 0 of every sample at 40x the others' norm (a BOS-like row), and
    a few -0.0 inputs in both halves."""
    g = torch.Generator().manual_seed(seed)
    kv = torch.randn(B, L, 2 * C, generator=g) * scale
    kv[:, 0] *= bos
    kv[:, min(3, L - 1), 0:2 * C:37] = -0.0
    kv[:, L - 1, 5] = -0.0
    kv[:, L - 1, C + 5] = -0.0
    return kv.to(BF).view(B * L, 2 * C)


def expand_ref(kv, B, L, C, heads, slots, col_off, scale):
    """out [B][heads * slots][C] bf16: (kv.float() * scale_f32).bfloat16() where j < L and the channel belongs to the head, +0
    elsewhere.  fp32 multiply then round-to-nearest-even is what pack2bf does: equality is exact."""
    d = C // heads
    val = (kv.view(B, L, 2 * C)[:, :, col_off:col_off + C].float() * torch.tensor(scale, dtype=torch.float32)).to(BF)
    out = torch.zeros(B, heads, slots, C, dtype=BF)
    for h in range(heads):
        out[:, h, :L, h * d:(h + 1) * d] = val[:, :, h * d:(h + 1) * d]
    return out.view(B, heads * slots, C)


# (B, L, C, heads, slots, col_off, scale)
EXPAND_CASES = [
    (1, 77, 320, 8, 80, 0, rsqrt_f32(40)),        # the 128-thread stride covers 256 channels: the second pass is partial
    (3, 77, 640, 8, 80, 640, 1.0),                # the V half
    (2, 77, 1280, 20, 80, 0, rsqrt_f32(64)),      # SD 2 (1 / 8)
    (1, 65, 320, 8, 80, 0, rsqrt_f32(40)),        # the smallest L the fused form takes
    (1, 80, 320, 8, 80, 320, 1.0),                # no pad slot
    (3, 4, 320, 8, 4, 0, rsqrt_f32(40)),          # image prompt: every slot used
    (2, 4, 64, 2, 16, 64, f32(0.6)),              # slots 4..15 of either head padded; the adapter scale on V
    (1, 4, 32, 1, 32, 0, rsqrt_f32(32)),
]


@pytest.mark.parametrize("B,L,C,heads,slots,col_off,scale", EXPAND_CASES)
def test_xattn_expand_bit_for_bit(sdlib, B, L, C, heads, slots, col_off, scale):
    kv = make_kv(B, L, C, seed=B * 100000 + L * 1000 + C + heads)
    out = guarded((B * heads * slots, C), BF, label="expansion")
    _lib.check(sdlib.sd_op_xattn_expand(stream(), P(guarded_input(kv, label="kv")), P(out), B, L, C, heads, slots, col_off, scale),
               "sd_op_xattn_expand")
    torch.cuda.synchronize()
    check_guards()
    ref = expand_ref(kv, B, L, C, heads, slots, col_off, scale)
    got = out.cpu().view(B, heads * slots, C)
    assert (bits(ref) == -32768).any(), "the case must carry a -0.0 through the expansion"
    diff = bits(got) != bits(ref)
    where = torch.nonzero(diff)[:1].tolist()
    assert not diff.any(), f"xattn_expand: {int(diff.sum())} of {diff.numel()} elements differ, the first at (b, row, c) = {where}"


# (B, R, Cc, perm16)
TRANSPOSE_CASES = [(2, 640, 320, 1), (1, 32, 320, 0), (3, 50, 70, 0), (1, 16, 8, 1), (2, 1600, 1280, 0)]


@pytest.mark.parametrize("B,R,Cc,perm", TRANSPOSE_CASES)
def test_transpose_bf16_bit_for_bit(sdlib, B, R, Cc, perm):
    src = random_bits((B, R, Cc), seed=R * 10000 + Cc)
    dst = guarded((B * Cc, R), BF, label="transposed")
    _lib.check(sdlib.sd_op_transpose_bf16(stream(), P(guarded_input(src.view(B * R, Cc), label="src")), P(dst), B, R, Cc, perm),
               "sd_op_transpose_bf16")
    torch.cuda.synchronize()
    check_guards()
    r = torch.arange(R)
    ref = torch.empty(B, Cc, R, dtype=torch.int16)
    ref[:, :, perm16(r) if perm else r] = bits(src).transpose(1, 2)
    diff = bits(dst).view(B, Cc, R) != ref
    assert not diff.any(), (f"transpose_bf16 perm16={perm}: {int(diff.sum())} of {diff.numel()} elements differ, the first at "
                            f"(b, c, r) = {torch.nonzero(diff)[:1].tolist()}")


def test_transpose_bf16_refuses_the_permutation_on_rows_that_are_no_multiple_of_16(sdlib):
    src = guarded_input(random_bits((24, 32), seed=1), label="src")
    dst = guarded((32, 24), BF, label="transposed")
    with pytest.raises(_lib.SdHipError, match="multiple of 16"):
        _lib.check(sdlib.sd_op_transpose_bf16(stream(), P(src), P(dst), 1, 24, 32, 1))
    torch.cuda.synchronize()
    assert torch.isnan(dst.float()).all()
    check_guards()


# (B, R, K, RT)
RETILE_CASES = [
    (2, 640, 320, 640),     # A^T: one row tile per sample
    (2, 320, 640, 32),      # Bw
    (1, 32, 32, 32),        # one tile
    (3, 64, 96, 16),
    (1, 48, 32, 16),        # 192 chunks: less than one block
]


@pytest.mark.parametrize("B,R,K,RT", RETILE_CASES)
def test_retile32_bit_for_bit(sdlib, B, R, K, RT):
    src = random_bits((B, R, K), seed=R * 10000 + K + RT)
    dst = guarded((B * R, K), BF, label="tiled")
    _lib.check(sdlib.sd_op_retile32(stream(), P(guarded_input(src.view(B * R, K), label="src")), P(dst), B, R, K, RT), "sd_op_retile32")
    torch.cuda.synchronize()
    check_guards()
    ref = bits(retile32_ref(src, B, R, K, RT)).view(B * R, K)
    diff = bits(dst) != ref
    assert not diff.any(), f"retile32: {int(diff.sum())} of {diff.numel()} elements differ, the first at {torch.nonzero(diff)[:1].tolist()}"
    assert same_bits(untile32(dst.cpu(), B, R, K, RT), src)


def test_retile32_refusals_write_nothing(sdlib):
    src = guarded_input(random_bits((64, 96), seed=2), label="src")
    dst = guarded((64, 96), BF, label="tiled")
    for R, K, RT, word in ((64, 48, 16, "K=48"), (64, 96, 24, "RT=24"), (60, 96, 16, "R=60"), (64, 96, 0, "RT=0")):
        with pytest.raises(_lib.SdHipError, match=word):
            _lib.check(sdlib.sd_op_retile32(stream(), P(src), P(dst), 1, R, K, RT))
    torch.cuda.synchronize()
    assert torch.isnan(dst.float()).all()
    check_guards()


# ---- b. sd_op_xattn_fold, stage by stage ---------------------------------------------------------------------------------------

# (UB, L, C, heads, tiled, norm2 folded)
FOLD_CASES = [
    (2, 77, 320, 8, True, True),
    (1, 77, 640, 8, True, False),
    (3, 77, 1280, 8, False, True),
    (2, 77, 1280, 20, False, True),       # 1600 key slots
    (1, 65, 320, 8, True, True),
    (1, 80, 640, 8, False, False),
]
FOLD_IDS = [f"UB{u}-L{l}-C{c}-h{h}-{'tiled' if t else 'plain'}-{'ln' if n else 'noln'}" for u, l, c, h, t, n in FOLD_CASES]


class FoldCase:
    """Inputs of one layer as the packer (csrc/pack.hip, the attn2 block) hands them to set_context: wqT = to_q transposed
    ([in][out]) and rounded; with norm2 folded, W[c][j] = W_q[j][c] gamma[c] - mean_c(W_q[j][c] gamma[c]) in fp64, to fp32, to
    bf16, and lnu[j] = sum_c W_q[j][c] beta[c] (fp64, to fp32); ones = 1.0f.  wo = to_out rounded."""

    def __init__(self, UB, L, C, heads, tiled, ln):
        self.UB, self.L, self.C, self.heads, self.tiled, self.ln = UB, L, C, heads, tiled, ln
        self.NP, self.d = heads * 80, C // heads
        g = torch.Generator().manual_seed(UB * 100000 + L * 1000 + C + heads + (7 if ln else 0))
        self.kv = make_kv(UB, L, C, seed=UB * 100000 + L * 1000 + C + heads + 1)
        self.wq = torch.randn(C, C, generator=g) / math.sqrt(C)
        self.wo = torch.randn(C, C, generator=g) / math.sqrt(C)
        self.gamma = 1.0 + 0.3 * torch.randn(C, generator=g)
        self.beta = 0.3 * torch.randn(C, generator=g)
        self.bo = torch.randn(C, generator=g)
        if ln:
            wg = self.wq.double() * self.gamma.double()[None, :]                       # [out j][in c]
            self.wqT = (wg - wg.mean(1, keepdim=True)).float().t().contiguous().to(BF)
            self.lnu = (self.wq.double() @ self.beta.double()).float().contiguous()
            self.ones = torch.ones(C) if not tiled else None
        else:
            self.wqT = self.wq.t().contiguous().to(BF)
            self.lnu = self.ones = None
        self.wo16 = self.wo.to(BF)
        self.scale = rsqrt_f32(self.d)

    def sample(self, b):
        """The same layer for sample b alone."""
        c = object.__new__(FoldCase)
        c.__dict__.update(self.__dict__)
        c.UB, c.kv = 1, self.kv.view(self.UB, self.L, 2 * self.C)[b].reshape(self.L, 2 * self.C).contiguous()
        return c


def run_fold(sdlib, c):
    """One sd_op_xattn_fold into fresh guarded buffers.  Returns the device tensors (at, bw, c1, c2, scratch [3][UB * NP][C])."""
    UB, NP, C = c.UB, c.NP, c.C
    at = guarded((UB * NP, C), BF, label="at")
    bw = guarded((UB * C, NP), BF, label="bw")
    c1 = guarded((UB, NP), torch.float32, label="c1") if c.ones is not None else None
    c2 = guarded((UB, NP), torch.float32, label="c2") if c.lnu is not None else None
    scratch = guarded((3 * UB * NP, C), BF, label="scratch")
    ops = [guarded_input(c.kv, label="kv"), guarded_input(c.wqT, label="wqT"), guarded_input(c.wo16, label="wo"),
           guarded_input(c.lnu, label="lnu") if c.lnu is not None else None,
           guarded_input(c.ones, label="ones") if c.ones is not None else None]
    args = [P(t) if t is not None else None for t in ops + [at, bw, c1, c2, scratch]]
    for k in range(2):      # the second call into the same buffers must leave the same bits
        _lib.check(sdlib.sd_op_xattn_fold(stream(), *args, UB, c.L, C, c.heads, 1 if c.tiled else 0), "sd_op_xattn_fold")
        torch.cuda.synchronize()
        if k == 0:
            first = [t.clone() if t is not None else None for t in (at, bw, c1, c2, scratch)]
    check_guards()
    for name, a, b in zip(("at", "bw", "c1", "c2", "scratch"), first, (at, bw, c1, c2, scratch)):
        assert a is None or same_bits(a, b), f"xattn_fold: a second call into the same buffers changed {name}"
    return at, bw, c1, c2, scratch.view(3, UB * NP, C)


def masked_product(x_exp, w, UB, heads, slots, L, C):
    """fp64 product (and magnitude) of a masked expansion [UB][heads * slots][C] with w [N][C]: row (h, j) holds head h's d
    channels only and rows j >= L are zero, so head by head over the live rows; the other rows stay exactly 0."""
    d = C // heads
    ref = torch.zeros(UB, heads, slots, w.shape[0], dtype=torch.float64)
    mag = torch.zeros_like(ref)
    xe = x_exp.view(UB, heads, slots, C)
    for h in range(heads):
        r, m = gemm_ref(xe[:, h, :L, h * d:(h + 1) * d].reshape(UB * L, d), w[:, h * d:(h + 1) * d])
        ref[:, h, :L], mag[:, h, :L] = r.view(UB, L, -1), m.view(UB, L, -1)
    return ref.view(UB, heads * slots, -1), mag.view(UB, heads * slots, -1)


def pad_rows(t, heads, slots, L):
    """The rows of the pad slots j >= L of every head: [..., heads * slots, C] -> [..., heads, slots - L, C]"""
    return t.reshape(*t.shape[:-2], heads, slots, t.shape[-1])[..., L:, :]


def natural_operands(c, at, bw, scratch):
    """(A^T [UB][NP][C], B^T [UB][NP][C]) in natural order as bf16 CPU tensors, un-tiled / un-permuted / transposed from what
    the launcher stored in at and bw."""
    UB, NP, C = c.UB, c.NP, c.C
    at, bw = at.cpu(), bw.cpu()
    if c.tiled:
        at_n = untile32(at, UB, NP, C, NP)
        bw_p = untile32(bw, UB, C, NP, 32)                              # [UB][C][permuted slot]
        bw_n = bw_p[:, :, perm16(torch.arange(NP))]                      # natural slot r sits at perm16(r)
    else:
        at_n, bw_n = at.view(UB, NP, C), bw.view(UB, C, NP)
    return at_n, bw_n.transpose(1, 2).contiguous()


@pytest.fixture(scope="module")
def fold_runs():
    """Every case is built on the device once and shared by the stage test and the consumer test (which keeps no guards on it)."""
    cache = {}

    def get(i):
        if i not in cache:
            c = FoldCase(*FOLD_CASES[i])
            cache[i] = (c, run_fold(_lib.load(), c))
        return cache[i]
    return get


@pytest.mark.parametrize("i", range(len(FOLD_CASES)), ids=FOLD_IDS)
def test_xattn_fold_stage_by_stage(sdlib, fold_runs, i):
    """Every stage from the launcher's own stored intermediates.  The two GEMMs against linear_bound with k_eff = C + 3, which is
    gemm_bound of the full expansion (its zero entries add nothing to the fp64 product or its magnitude).  c1: linear_bound with
    k_eff = C over the ROUNDED row of at (the products with 1.0f are exact).  c2: k_eff = C + 1 -- lnu is fp32, so each product
    is rounded once before the C - 1 additions.  c1 a second time under the bound of gemv_kernel's own summation order (below),
    with the assertion that the row sums of the unrounded product fall outside it.  Measured worst err / bound on an MI355X over
    FOLD_CASES: both GEMMs 0.486 .. 0.498 (the output rounding), c2 5.6e-4 .. 3.8e-3, c1 5.4e-5 / 5.8e-5 under k_eff = C and
    4.1e-3 / 4.4e-3 under the depth bound; the unrounded product's row sums sit at a median of 40 bounds, 1825 of 1848 and 3038
    of 3080 live slots outside."""
    c, (at, bw, c1, c2, scratch) = fold_runs(i)
    UB, L, C, heads, NP = c.UB, c.L, c.C, c.heads, c.NP
    what = f"xattn_fold {FOLD_IDS[i]}"
    kexp = expand_ref(c.kv, UB, L, C, heads, 80, 0, c.scale)
    vexp = expand_ref(c.kv, UB, L, C, heads, 80, C, 1.0)
    slab = scratch.cpu()
    # the V expansion, still in slab 1
    assert same_bits(slab[1].view(UB, NP, C), vexp), f"{what}: slab 1 is not the V expansion"
    # B^T in natural order, in slab 0
    bT = slab[0].view(UB, NP, C)
    r64, m64 = masked_product(vexp, c.wo16, UB, heads, 80, L, C)
    assert_elementwise(bT, r64, linear_bound(r64, m64, C + 3), what + " B^T (slab 0)", ("b", "slot", "c"))
    assert (bits(pad_rows(bT, heads, 80, L)) == 0).all(), f"{what}: a pad-slot row of B^T is not +0"
    # at and bw against the natural-order intermediates
    at_n, bw_n = natural_operands(c, at, bw, scratch)
    r64, m64 = masked_product(kexp, c.wqT, UB, heads, 80, L, C)
    a_exact = r64
    assert_elementwise(at_n, r64, linear_bound(r64, m64, C + 3), what + " A^T", ("b", "slot", "c"))
    assert (bits(pad_rows(at_n, heads, 80, L)) == 0).all(), f"{what}: a pad-slot row of A^T is not +0"
    assert same_bits(bw_n, bT), f"{what}: bw is not the (re-tiled, permuted) transpose of slab 0"
    if c.tiled:     # slab 2: the permuted transpose before its re-tiling
        assert same_bits(retile32_ref(slab[2].view(UB, C, NP), UB, C, NP, 32).view(UB * C, NP), bw.cpu()), f"{what}: slab 2"
    else:
        assert torch.isnan(slab[2].float()).all(), f"{what}: the plain form wrote the third slab"
    pad = torch.zeros(heads, 80, dtype=torch.bool)
    pad[:, L:] = True
    if c1 is not None:
        a64 = at_n.double()
        s64, sm = a64.sum(-1), a64.abs().sum(-1)
        assert_elementwise(c1, s64, linear_bound(s64, sm, C, torch.float32), what + " c1", ("b", "slot"))
        assert (c1.cpu().view(UB, heads, 80)[:, pad] == 0).all(), f"{what}: c1 of a pad slot is not 0"
        # k_eff = C is the worst case of ANY summation order; at C = 1280 it is as wide as the difference between the row sum
        # of the rounded row and that of the unrounded product (~ 2^-9 |a| sqrt(C) against 2^-24 C^2 |a|), which is the one
        # thing c1 exists to tell apart.  gemv_kernel's own order is known: a lane adds the eight products of a chunk left to
        # right (7 additions) and the chunk sum to its accumulator (ceil(C / 512) chunks per lane), then wave_sum's six
        # butterfly levels -- no term passes through more than 7 + ceil(C / 512) + 6 additions, and the products with 1.0f are
        # exact.  One more for the second-order terms of (1 + u)^depth.
        depth = 7 + -(-C // 512) + 6 + 1
        tight = linear_bound(s64, sm, depth, torch.float32)
        assert_elementwise(c1, s64, tight, what + " c1 (summation depth of gemv_kernel)", ("b", "slot"))
        # ... and under that bound the check discriminates: the row sums of the UNROUNDED product are outside it
        live = ~pad.view(-1)
        off = ((a_exact.sum(-1) - s64).abs() / tight)[:, live]
        print(f"[bounds] {what} c1 from the unrounded product: {int((off > 1).sum())} of {off.numel()} live slots outside the bound, "
              f"worst ratio {float(off.max()):.3g}, median {float(off.median()):.3g}")
        assert (off > 1).float().mean() > 0.5, f"{what}: the c1 bound cannot tell the rounded row from the unrounded product"
    if c2 is not None:
        u64 = c.lnu.double()
        s64, sm = kexp.double() @ u64, kexp.double().abs() @ u64.abs()
        assert_elementwise(c2, s64, linear_bound(s64, sm, C + 1, torch.float32), what + " c2", ("b", "slot"))
        assert (c2.cpu().view(UB, heads, 80)[:, pad] == 0).all(), f"{what}: c2 of a pad slot is not 0"
    # no cross-sample indexing: sample b alone reproduces its slice
    for b in range(UB if UB > 1 else 0):
        one = run_fold(sdlib, c.sample(b))
        for name, full, part in zip(("at", "bw", "c1", "c2"), (at, bw, c1, c2), one[:4]):
            if full is not None:
                assert same_bits(full.cpu().view(UB, -1)[b], part.cpu().view(-1)), f"{what}: {name} of sample {b} alone differs"
        for s in range(3):
            assert same_bits(slab[s].view(UB, -1)[b], one[4][s].cpu().view(-1)), f"{what}: slab {s} of sample {b} alone differs"


# ---- c. producer meets consumer --------------------------------------------------------------------------------------------------

HW = 128            # tokens per sample


def row_partials(x, C):
    """[parts][M][2]: (sum, sum of squares) of every 80-column slice, as a producer's epilogue delivers them."""
    xs = x.double().view(x.shape[0], C // 80, 80)
    return torch.stack([xs.sum(-1), (xs * xs).sum(-1)], -1).permute(1, 0, 2).float().contiguous()


@pytest.mark.parametrize("i", range(len(FOLD_CASES)), ids=FOLD_IDS)
def test_device_built_operands_feed_the_consumer_kernels(sdlib, fold_runs, i):
    """The device-built at / bw / c1 / c2 go straight into the kernels that consume them in the UNet: sd_op_xattn_fused(_ln) for
    the tiled form, sd_op_gemm_batched(_softmax_ln) + sd_op_gemm_batched for the plain one.  No Python code restates the tiling
    here: the per-element references take A^T and B^T in natural order from a plain-form run of the same launcher on the same
    inputs (B^T: slab 0).  Per element: xattn_elementwise / xattn_norm2_elementwise; the plain form with norm2 folded carries the
    c1 term, so its scores and their error come from ln_fold_ref_bound and enter xattn_elementwise as S and S_abs_err.
    rel-L2: 8e-3 against the folded formula in fp64 from the device-built operands, 2e-2 against LayerNorm +
    F.scaled_dot_product_attention + linears on the unfolded fp32 weights (the two thresholds of test_xattn_fused).  Measured on
    an MI355X, in FOLD_CASES' order: worst err / bound 0.229, 0.113, 0.062, 0.028, 0.187, 0.113; rel-L2 1.7e-3 against the
    folded formula in every case, 5.9e-3 .. 9.5e-3 against the unfolded attention."""
    c, (at, bw, c1, c2, scratch) = fold_runs(i)
    UB, L, C, heads, NP, d = c.UB, c.L, c.C, c.heads, c.NP, c.d
    M = UB * HW
    what = f"fold -> consumer {FOLD_IDS[i]}"
    g = torch.Generator().manual_seed(4000 + i)
    x = (torch.randn(M, C, generator=g) * 0.8 + (0.5 if c.ln else 0.0) + 0.3 * torch.randn(M, 1, generator=g)).to(BF)
    r = torch.randn(M, C, generator=g).to(BF)
    xd, rd, bod = guarded_input(x, label="x"), guarded_input(r, label="r"), guarded_input(c.bo, label="bias")
    out = guarded((M, C), BF, label="y")
    rs = row_partials(x, C) if c.ln else None
    parts = rs.shape[0] if c.ln else 0
    if c.tiled and c.ln:
        ors = guarded((sdlib.sd_op_ln_partials(1, M, C), M, 2), torch.float32, label="rowstats")
        _lib.check(sdlib.sd_op_xattn_fused_ln(stream(), P(xd), P(rd), P(out), P(at), P(bw), P(bod), M, C, HW, L,
                                              P(guarded_input(rs, label="ln partials")), parts, M, P(c2), 1e-5, P(ors)),
                   "sd_op_xattn_fused_ln")
    elif c.tiled:
        _lib.check(sdlib.sd_op_xattn_fused(stream(), P(xd), P(rd), P(out), P(at), P(bw), P(bod), M, C, HW, L), "sd_op_xattn_fused")
    else:
        pr = guarded((M, NP), BF, label="probabilities")
        if c.ln:
            _lib.check(sdlib.sd_op_gemm_batched_softmax_ln(stream(), P(xd), C, P(at), NP * C, HW, P(pr), NP, M, NP, C, L,
                                                           P(guarded_input(rs, label="ln partials")), parts, P(c1), P(c2), 1e-5),
                       "sd_op_gemm_batched_softmax_ln")
        else:
            _lib.check(sdlib.sd_op_gemm_batched(stream(), P(xd), C, P(at), NP * C, HW, None, None, NP, P(pr), NP, M, NP, C, 2, L),
                       "sd_op_gemm_batched (softmax)")
        _lib.check(sdlib.sd_op_gemm_batched(stream(), P(pr), NP, P(bw), C * NP, HW, P(bod), P(rd), C, P(out), C, M, C, NP, 0, 0),
                   "sd_op_gemm_batched")
    torch.cuda.synchronize()
    check_guards()
    assert torch.isfinite(out.float()).all()
    # natural-order operands from the device: B^T = slab 0; A^T = at of the plain form
    Bn = scratch[0].cpu().view(UB, NP, C).float()
    if c.tiled:
        pc = object.__new__(FoldCase)
        pc.__dict__.update(c.__dict__)
        pc.tiled, pc.ones = False, None
        at_plain, _, _, _, sp = run_fold(sdlib, pc)
        assert same_bits(sp[0], scratch[0]), f"{what}: the plain form built another B^T"
        An = at_plain.cpu().view(UB, NP, C).float()
    else:
        An = at.cpu().view(UB, NP, C).float()
    x64 = x.double().view(UB, HW, C)
    c2h = c2.cpu() if c2 is not None else None
    if c.ln and c.tiled:
        xattn_norm2_elementwise(out.cpu(), x.float(), An, c2h, rs, Bn, r.float(), c.bo, L, UB, HW, C, M, what)
    elif c.ln:
        tot = rs.double().sum(0)
        zs, dzs = zip(*(ln_fold_ref_bound(x.float()[b * HW:(b + 1) * HW], An[b], c1.cpu()[b], c2h[b], tot[b * HW:(b + 1) * HW, 0],
                                          tot[b * HW:(b + 1) * HW, 1], 1e-5) for b in range(UB)))
        S, dS = torch.stack(zs), torch.stack(dzs)
        xattn_elementwise(out.cpu().view(UB, HW, C), S, torch.zeros_like(S), 0.0, Bn, r.float(), c.bo, L, what, S_abs_err=dS)
    else:
        xattn_elementwise(out.cpu().view(UB, HW, C), torch.einsum("bmc,bkc->bmk", x64, An.double()),
                          torch.einsum("bmc,bkc->bmk", x64.abs(), An.double().abs()), U32 * (C + 2), Bn, r.float(), c.bo, L, what)
    # rel-L2 (i): the folded formula in fp64 from the device-built operands
    if c.ln:
        mean = x.double().mean(-1, keepdim=True)
        rstd = 1.0 / torch.sqrt(x.double().var(-1, unbiased=False, keepdim=True) + 1e-5)
        S = rstd.view(UB, HW, 1) * torch.einsum("bmc,bkc->bmk", x64, An.double()) + c2h.double()[:, None, :]
        if c1 is not None:
            S = S - (rstd * mean).view(UB, HW, 1) * c1.cpu().double()[:, None, :]
        xn = ((x.double() - mean) * rstd * c.gamma.double() + c.beta.double()).float().view(UB, HW, C)
    else:
        S = torch.einsum("bmc,bkc->bmk", x64, An.double())
        xn = x.float().view(UB, HW, C)
    Sg = S.view(UB, HW, heads, 80).clone()
    Sg[..., L:] = float("-inf")
    Pm = torch.softmax(Sg, -1).view(UB, HW, NP)
    ref_fold = (r.double().view(UB, HW, C) + torch.einsum("bmk,bkc->bmc", Pm, Bn.double()) + c.bo.double()).view(M, C)
    # (ii) the unfolded attention on the fp32 weights
    K, V = (c.kv.float().view(UB, L, 2 * C)[:, :, o:o + C].view(UB, L, heads, d).transpose(1, 2) for o in (0, C))
    q = (xn @ c.wq.t()).view(UB, HW, heads, d).transpose(1, 2)
    o = F.scaled_dot_product_attention(q, K, V).transpose(1, 2).reshape(UB, HW, C)
    ref_attn = (r.float().view(UB, HW, C) + o @ c.wo.t() + c.bo).view(M, C)
    e1, e2 = rel_l2(out, ref_fold), rel_l2(out, ref_attn)
    print(f"{what}: vs folded fp64 {e1:.3e}, vs SDPA + linears {e2:.3e}")
    assert e1 < 8e-3 and e2 < 2e-2


# ---- d. sd_op_ip_fold -----------------------------------------------------------------------------------------------------------

T_IP = 4
# (UB, C, heads, scale)
IP_CASES = [(2, 320, 8, 1.0), (1, 1280, 8, f32(0.6)), (3, 64, 2, 1.0),
            (1, 32, 1, 0.0),        # the two GEMMs take K = C as a multiple of 64: refused by name, nothing launched
            (1, 64, 1, 0.0)]        # one head over all 32 slots, adapter scale 0


def run_ip_fold(sdlib, kv, wqT, wo16, UB, C, heads, scale):
    at = guarded((UB * 32, C), BF, label="A")
    bt = guarded((UB * C, 32), BF, label="Bt")
    scratch = guarded((3 * UB * 32, C), BF, label="scratch")
    args = [P(guarded_input(kv, label="ip_kv")), P(guarded_input(wqT, label="wqT")), P(guarded_input(wo16, label="wo")), P(at), P(bt),
            P(scratch)]
    for k in range(2):
        _lib.check(sdlib.sd_op_ip_fold(stream(), *args, UB, T_IP, C, heads, scale), "sd_op_ip_fold")
        torch.cuda.synchronize()
        if k == 0:
            first = [t.clone() for t in (at, bt, scratch)]
    check_guards()
    for name, a, b in zip(("A", "Bt", "scratch"), first, (at, bt, scratch)):
        assert same_bits(a, b), f"ip_fold: a second call into the same buffers changed {name}"
    return at, bt, scratch.view(3, UB * 32, C)


def ip_fold_inputs(UB, C, heads, family):
    """(ip_kv [UB * 4][2 C] bf16, W_q, W_o fp32).  ``dense``: noise everywhere, as in the UNet.  ``sharp``: the operand family of
    tests/ip_xattn_case.py under which its worst-case bound is a few per cent of the image branch, built THROUGH the fold --
    W_q = 1, one live K channel per (token, head) so that a row of A lives on one channel (amplitude 2), and output channel c
    of W_o reads head c mod heads alone, so that a column of Bt listens to one head."""
    g = torch.Generator().manual_seed(UB * 10000 + C + heads + (3 if family == "sharp" else 0))
    d = C // heads
    if family == "dense":
        kv = make_kv(UB, T_IP, C, seed=UB * 10000 + C + heads + 1, scale=1.5, bos=1.0)
        wq, wo = (torch.randn(C, C, generator=g) / math.sqrt(C) for _ in range(2))
        return kv, wq, wo
    kv = torch.zeros(UB, T_IP, heads, 2, d)
    chan = torch.randint(0, d, (UB, T_IP, heads, 1), generator=g)
    kv[:, :, :, 0].scatter_(-1, chan, 2.0 * math.sqrt(d) * torch.randn(UB, T_IP, heads, 1, generator=g))
    kv[:, :, :, 1] = 1.5 * torch.randn(UB, T_IP, heads, d, generator=g)
    kv = kv.permute(0, 1, 3, 2, 4).reshape(UB * T_IP, 2 * C).to(BF)                    # [token][K | V][head][d]
    listens = (torch.arange(C)[None, :] // d == torch.arange(C)[:, None] % heads).float()      # [out c][in k]
    wo = torch.randn(C, C, generator=g) * (0.33 / math.sqrt(d)) * listens
    return kv, torch.eye(C), wo


@pytest.mark.parametrize("family", ["dense", "sharp"])
@pytest.mark.parametrize("UB,C,heads,scale", IP_CASES)
def test_ip_fold_stage_by_stage_and_into_ip_xattn(sdlib, UB, C, heads, scale, family):
    """The stage checks of test_xattn_fold_stage_by_stage over 32 key slots (32 / heads per head, 4 image tokens), then the
    device-built A / Bt go straight into sd_op_ip_xattn under tests/ip_xattn_case.py's bound (on ``dense`` operands that bound is
    wider than the branch and sees addressing and finiteness; ``sharp``, see ip_fold_inputs, is where a wrong slot, head or
    transpose shows).  scale = 0: Rout == R bit for bit.  Measured worst err / bound on an MI355X: both GEMMs 0.48 .. 0.50;
    into ip_xattn 0.03 .. 0.13 dense, 0.475 .. 0.491 sharp.
    C = 32 cannot be folded: sd_launch_gemm takes K as a multiple of 64 and no UNet level is narrower, so the launcher refuses
    it by name before its first launch; C = 64 with one head stands in for it as the scale-0 case that runs."""
    from tests.ip_xattn_case import EPS, operands, ref_bound
    if C % 64:
        at, bt, scratch = (guarded((n, m), BF, label=l) for n, m, l in ((UB * 32, C, "A"), (UB * C, 32, "Bt"), (3 * UB * 32, C, "scratch")))
        kv = guarded_input(make_kv(UB, T_IP, C, seed=5), label="ip_kv")
        w = guarded_input(torch.eye(C).to(BF), label="w")
        with pytest.raises(_lib.SdHipError, match=f"ip_fold: C={C} must be a multiple of 64"):
            _lib.check(sdlib.sd_op_ip_fold(stream(), P(kv), P(w), P(w), P(at), P(bt), P(scratch), UB, T_IP, C, heads, scale))
        torch.cuda.synchronize()
        assert all(torch.isnan(t.float()).all() for t in (at, bt, scratch))
        check_guards()
        return
    sph, d, rps = 32 // heads, C // heads, 40
    what = f"ip_fold {family} UB={UB} C={C} heads={heads} scale={scale:g}"
    kv, wq, wo = ip_fold_inputs(UB, C, heads, family)
    wqT, wo16 = wq.t().contiguous().to(BF), wo.to(BF)
    at, bt, scratch = run_ip_fold(sdlib, kv, wqT, wo16, UB, C, heads, scale)
    slab = scratch.cpu()
    kexp = expand_ref(kv, UB, T_IP, C, heads, sph, 0, rsqrt_f32(d))
    vexp = expand_ref(kv, UB, T_IP, C, heads, sph, C, scale)
    assert same_bits(slab[0].view(UB, 32, C), kexp), f"{what}: slab 0 is not the K expansion"
    assert same_bits(slab[1].view(UB, 32, C), vexp), f"{what}: slab 1 is not the V expansion"
    bT, A = slab[2].view(UB, 32, C), at.cpu().view(UB, 32, C)
    r64, m64 = masked_product(vexp, wo16, UB, heads, sph, T_IP, C)
    assert_elementwise(bT, r64, linear_bound(r64, m64, C + 3), what + " B^T (slab 2)", ("b", "slot", "c"))
    r64, m64 = masked_product(kexp, wqT, UB, heads, sph, T_IP, C)
    assert_elementwise(A, r64, linear_bound(r64, m64, C + 3), what + " A", ("b", "slot", "c"))
    if sph > T_IP:
        assert (bits(pad_rows(bT, heads, sph, T_IP)) == 0).all() and (bits(pad_rows(A, heads, sph, T_IP)) == 0).all(), \
            f"{what}: a pad-slot row is not +0"
    assert same_bits(bt.cpu().view(UB, C, 32), bT.transpose(1, 2).contiguous()), f"{what}: Bt is not the transpose of slab 2"
    for b in range(UB if UB > 1 else 0):
        one = run_ip_fold(sdlib, kv.view(UB, T_IP, 2 * C)[b].contiguous(), wqT, wo16, 1, C, heads, scale)
        for name, full, part in zip(("A", "Bt"), (at, bt), one[:2]):
            assert same_bits(full.cpu().view(UB, -1)[b], part.cpu().view(-1)), f"{what}: {name} of sample {b} alone differs"
    # consumer
    r, _, _, gamma, beta = operands(UB, rps, C, heads, "dense")
    M = UB * rps
    rd = guarded_input(r, BF, label="R")
    out = guarded((M, C), BF, label="Rout")
    _lib.check(sdlib.sd_op_ip_xattn(stream(), P(rd), P(out), P(at), P(bt), P(guarded_input(gamma, label="gamma")),
                                    P(guarded_input(beta, label="beta")), EPS, M, C, rps, heads, T_IP), "sd_op_ip_xattn")
    torch.cuda.synchronize()
    check_guards()
    y, bound, branch = ref_bound(r, A.float(), bt.cpu().view(UB, C, 32).float(), gamma, beta, EPS, UB, rps, C, heads)
    assert_elementwise(out.float().cpu().view(UB, rps, C), y, bound, what + " -> ip_xattn", ("b", "row", "c"))
    if scale == 0.0:
        assert same_bits(out, rd), f"{what}: an adapter scale of 0 must leave the residual as it is"
    else:
        assert (out.float() - rd.float()).abs().max().item() > 0.05, "the image branch must move the residual in this test"


# ---- e. refusals by name that launch nothing ------------------------------------------------------------------------------------

def test_fold_refusals_launch_nothing(sdlib):
    C, NP = 320, 640
    kv = guarded_input(make_kv(1, 77, C, seed=9), label="kv")
    w = guarded_input((torch.randn(C, C, generator=torch.Generator().manual_seed(9)) / 18).to(BF), label="w")
    vec = guarded_input(torch.ones(C), label="vector")
    at, bw = guarded((NP, C), BF, label="at"), guarded((C, NP), BF, label="bw")
    c1, c2 = guarded((1, NP), torch.float32, label="c1"), guarded((1, NP), torch.float32, label="c2")
    scratch = guarded((3 * NP, C), BF, label="scratch")
    ex = guarded((NP, C), BF, label="expansion")
    outs = (at, bw, c1, c2, scratch, ex)
    s = stream()

    def fold(kv_=P(kv), wq_=P(w), wo_=P(w), lnu=None, ones=None, at_=P(at), bw_=P(bw), c1_=None, c2_=None, sc=P(scratch), UB=1, L=77,
             C_=C, heads=8, perm=0):
        return sdlib.sd_op_xattn_fold(s, kv_, wq_, wo_, lnu, ones, at_, bw_, c1_, c2_, sc, UB, L, C_, heads, perm)

    def ipf(kv_=P(kv), wq_=P(w), wo_=P(w), at_=P(at), bt_=P(bw), sc=P(scratch), UB=1, T=4, C_=C, heads=8, scale=1.0):
        return sdlib.sd_op_ip_fold(s, kv_, wq_, wo_, at_, bt_, sc, UB, T, C_, heads, scale)

    refusals = [
        (lambda: fold(kv_=None), "xattn_fold: null operand"), (lambda: fold(wo_=None), "xattn_fold: null operand"),
        (lambda: fold(at_=None), "xattn_fold: null operand"), (lambda: fold(sc=None), "xattn_fold: null operand"),
        (lambda: fold(lnu=P(vec)), "c2 with lnu"), (lambda: fold(c1_=P(c1)), "c1 goes with ones"),
        (lambda: fold(ones=P(vec), c1_=P(c1), perm=1), "tiled form takes none"),
        (lambda: fold(L=81), "81 prompt keys"), (lambda: fold(L=0), "0 prompt keys"),
        (lambda: fold(heads=64), "odd head dim 5"), (lambda: fold(heads=7), "heads=7 does not divide C=320"),
        (lambda: fold(C_=96, heads=8), "C=96 must be a multiple of 64"),
        (lambda: ipf(kv_=None), "ip_fold: null operand"), (lambda: ipf(bt_=None), "ip_fold: null operand"),
        (lambda: ipf(T=5), "5 image tokens"), (lambda: ipf(heads=64), "odd head dim 5"),
        (lambda: ipf(heads=7), "heads=7 does not divide C=320"), (lambda: ipf(C_=32, heads=1), "C=32 must be a multiple of 64"),
        (lambda: sdlib.sd_op_xattn_expand(s, None, P(ex), 1, 77, C, 8, 80, 0, 1.0), "xattn_expand"),
        (lambda: sdlib.sd_op_xattn_expand(s, P(kv), P(ex), 1, 5, C, 8, 4, 0, 1.0), "L=5 .* slots=4"),
        (lambda: sdlib.sd_op_xattn_expand(s, P(kv), P(ex), 1, 77, C, 64, 80, 0, 1.0), "heads=64"),
        (lambda: sdlib.sd_op_xattn_expand(s, P(kv), P(ex), 1, 77, C, 7, 80, 0, 1.0), "heads=7"),
        (lambda: sdlib.sd_op_xattn_expand(s, P(kv), P(ex), 1, 77, C, 8, 80, 40, 1.0), "col_off 40"),
        (lambda: sdlib.sd_op_transpose_bf16(s, None, P(ex), 1, 32, 32, 0), "transpose"),
        (lambda: sdlib.sd_op_retile32(s, P(kv), None, 1, 32, 32, 32), "retile32"),
    ]
    for call, word in refusals:
        with pytest.raises(_lib.SdHipError, match=word):
            _lib.check(call())
    torch.cuda.synchronize()
    for t in outs:
        assert torch.isnan(t.float()).all()          # nothing ran: every output still holds its fill
    check_guards()


# ---- 3. results must not depend on what the workspace held ----------------------------------------------------------------------

def fill_workspace(ws, kind):
    """Every byte of the workspace tensor: zeros, 0xFF, or the bf16 pattern 0x7FC0 from the 256-byte boundary the handles align
    their workspace to (NaN as bf16 and, two at a time, as fp32)."""
    if kind == "zeros":
        ws.zero_()
    else:
        ws.fill_(0xFF)
        if kind == "nan":
            off = (-ws.data_ptr()) % 256
            n = (ws.numel() - off) // 2 * 2
            ws[off:off + n].view(torch.int16).fill_(0x7FC0)
    torch.cuda.synchronize()


FILLS = ("zeros", "0xFF", "nan")


def assert_same_after_every_fill(outs, what):
    for kind, o in zip(FILLS, outs):
        assert torch.isfinite(o).all(), f"{what}: not finite after the workspace was filled with {kind}"
    for kind, o in zip(FILLS[1:], outs[1:]):
        diff = bits(o) != bits(outs[0])
        assert not diff.any(), (f"{what}: {int(diff.sum())} of {diff.numel()} outputs depend on what the workspace held "
                                f"({kind} against zeros), the first at {torch.nonzero(diff)[:1].tolist()}")


def unet_after_every_fill(net, lat, ctx, t, image=None):
    ub = ctx.shape[0]
    outs = []
    for kind in FILLS:
        fill_workspace(net._workspace(ub), kind)
        net.set_context(ctx)
        if image is not None:
            net.set_ip_adapter(*image)
        outs.append(net.forward_latents(lat, ub, t).clone().cpu())          # a full forward: no DeepCache skip, no T-GATE reuse
    return outs


def test_unet_with_all_three_prompt_attention_forms_ignores_old_workspace_contents():
    """A three-level UNet on 32x32 latents: 1024 tokens at 8 heads (the fused kernel), 256 tokens (the two per-sample GEMMs),
    64 tokens in the last level and the mid block (to_q + 77-key attention + to_out).  The form depends on a level's token and
    head count alone, so two levels cannot hold three forms.  The launch counts say which forms ran: 16 transformer blocks, 5 of
    them fused, 6 with a prompt attention launch of their own."""
    from sonicdiffusionbayeslab_amd.unet import HipUNet2DConditionModel
    from sonicdiffusionbayeslab_amd.weights import UNetConfig, make_synthetic_state_dict
    from tests.util import synth_inputs
    cfg = UNetConfig(sample_size=32, block_out_channels=(320, 320, 640), attn_levels=(True, True, True))
    net = HipUNet2DConditionModel(cfg, make_synthetic_state_dict(cfg, seed=99))
    lat, pe, ne = synth_inputs(cfg, 1, seed=41)
    ctx, x = torch.cat([ne, pe]).cuda(), lat.cuda()
    outs = unet_after_every_fill(net, x, ctx, 501.0)
    prof = net.forward_profiled(x, 2, 501.0)
    print(f"launches: xattn_fused {prof['xattn_fused']['launches']}, attention {prof['attention']['launches']}")
    assert prof["xattn_fused"]["launches"] == 5
    assert prof["attention"]["launches"] == 16 + 6          # every self-attention, and the prompt attention of six blocks
    assert_same_after_every_fill(outs, "three-level UNet")


def test_sd2_twenty_head_unet_ignores_old_workspace_contents():
    """The config of tests/test_sd2_gpu.py::test_folded_prompt_attention_at_twenty_heads_matches_oracle: 20 heads on 256 tokens
    (1600 key slots in the two-GEMM form)."""
    from sonicdiffusionbayeslab_amd.unet import HipUNet2DConditionModel
    from sonicdiffusionbayeslab_amd.weights import UNetConfig, make_synthetic_state_dict
    from tests.util import synth_inputs
    cfg = UNetConfig(sample_size=16, block_out_channels=(1280, 1280), attn_levels=(True, False), cross_attention_dim=1024,
                     num_heads=20, num_heads_per_level=(20, 20), use_linear_projection=True)
    net = HipUNet2DConditionModel(cfg, make_synthetic_state_dict(cfg, seed=77))
    lat, pe, ne = synth_inputs(cfg, 1, seed=71)
    ctx, x = torch.cat([ne, pe]).cuda(), lat.cuda()
    outs = unet_after_every_fill(net, x, ctx, 501.0)
    prof = net.forward_profiled(x, 2, 501.0)
    assert prof["attention"]["launches"] == 5 + 2 and "xattn_fused" not in prof
    assert_same_after_every_fill(outs, "SD 2 two-level UNet at 20 heads")


@pytest.fixture(scope="module")
def vae_weights():
    from sonicdiffusionbayeslab_amd.vae import VaeConfig, make_synthetic_vae_state_dict
    cfg = VaeConfig()
    return cfg, make_synthetic_vae_state_dict(cfg)


def test_vae_decoder_ignores_old_workspace_contents(vae_weights):
    """The AutoencoderKL decoder on a 16x16 latent."""
    from sonicdiffusionbayeslab_amd.vae import HipVaeDecoder
    lat = torch.randn(1, 4, 16, 16, generator=torch.Generator().manual_seed(17)).cuda()
    dec = HipVaeDecoder(*vae_weights)
    outs = []
    for kind in FILLS:
        fill_workspace(dec._workspace(1, 16, 16), kind)
        outs.append(dec.decode(lat).clone().cpu())
    assert_same_after_every_fill(outs, "VAE decoder 16x16")


def test_vae_encoder_ignores_old_workspace_contents(vae_weights):
    """The AutoencoderKL encoder on a 64x64 image, its smallest."""
    from sonicdiffusionbayeslab_amd.vae import HipVaeEncoder
    img = torch.rand(1, 3, 64, 64, generator=torch.Generator().manual_seed(18)).cuda()
    enc = HipVaeEncoder(*vae_weights)
    outs = []
    for kind in FILLS:
        fill_workspace(enc._workspace(1, 8, 8), kind)
        outs.append(enc.encode(img).clone().cpu())
    assert_same_after_every_fill(outs, "VAE encoder 64x64")
