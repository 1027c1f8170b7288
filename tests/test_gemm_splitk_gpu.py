"""GPU: gemm_kernel's persistent (output tile x K split) work loop and splitk_reduce_kernel (csrc/gemm_conv.hip), per element
against fp64, beyond one row tile: split-K on the 64-row tile, several M tiles, M and N tails, a grid that is no multiple of
8 (the r != 0 branch of the XCD map), more than 512 items (a workgroup walks from one item to another with a different
kt_begin, the next item's first K tile prefetched before the epilogue), a split that straddles K1, pitched ldx / ldx2 / ldr /
ldc in the reduce -- through sd_op_gemm and, for AMODE_CONV on the same loop, sd_op_conv3x3.  The cases and the properties
each exists for are tests/gemm_cases.py; tests/test_gemm_dispatch_cpu.py pins their variants without a GPU, and every test
here first asserts, through the library's dispatch report, the variant the table says (a retune must not quietly turn these
into no-split cases).

Inputs are bf16-rounded randn, weights scaled by 1 / sqrt(K); every operand sits between NaN-poisoned guards, the output is
NaN-prefilled between sentinel guards (tests/bounds.py) and check_guards() follows every launch.  The gate is the project's
a-priori bound (gemm_bound / linear_bound): one output ulp + the worst-case fp32 summation of K + 3 terms, so a correct kernel
sits near 0.5 and one K tile of one item counted twice or dropped is ~100 x the bound (tests/test_bounds_cpu.py).

With SD_SPLITK / SD_GEMM_SMALL / SD_GEMM_BIG / SD_GEMM_LEAN set the variants are not the product's: the file skips.

Measured on an MI355X (rows / split / items as the library reports them; worst |err| / bound; no guard touched, no case failed):
  77 x 768 x 3072          64 / 4 / 40    0.409  (pitched: 0.409)      3072 x 640 x 2560   64 / 3 / 576   0.457  (two launches equal)
  257 x 1024 x 4096        64 / 5 / 175   0.375                         3000 x 640 x 2560   64 / 3 / 564   0.430
  128 x 1280 x 5120        64 / 6 / 96    0.342                         6144 x 1280 x 1536  128 / 2 / 768  0.465
  514 x 1280 x 5120        64 / 6 / 432   0.343                         10817 x 160 x 2560 (K1 1280)  64 / 3 / 510  0.430
  192 x 1280 x 2560 (1280) 64 / 3 / 72    0.457  (pitched: 0.457)      conv 2 x 64 x 64, 320 -> 320, stride 2    128 / 3 / 96   0.447
  192 x 640 x 1920 (1280)  64 / 2 / 24    0.447                         conv 4 x 128 x 128, 192 -> 480, stride 2  128 / 2 / 768  0.467
  200 x 324 x 1536         64 / 2 / 24    0.464
  fp8 (tests/test_fp8_gpu.py::test_gemm_fp8): 300 x 1280 x 5120 128 / 3 / 72 0.399; 257 x 1024 x 4096 128 / 2 / 42 0.376;
  6144 x 1280 x 3072 128 / 2 / 768 0.414
Every ratio is below 0.5: the output rounding alone."""
import math
import os

import pytest
import torch

from sonicdiffusionbayeslab_amd import _lib
from tests.bounds import (NHWC, assert_elementwise, check_guards, conv3x3_nhwc_ref, forget_guards, gemm_bound, guarded,
                          guarded_input, linear_bound)
from tests.gemm_cases import (CONV_CASES, FAULT_CASE, GEMM_CASES, GEMM_DETERMINISM, GEMM_PITCHED, case_id, conv_dims, derive,
                              holds)

SELECTORS = ("SD_SPLITK", "SD_GEMM_SMALL", "SD_GEMM_BIG", "SD_GEMM_LEAN")
_set = [v for v in SELECTORS if v in os.environ]
pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(bool(_set), reason=f"{', '.join(_set)} set: the GEMM variants are not the product's")]


def stream():
    return torch.cuda.current_stream().cuda_stream


def r16(t):
    return t.to(torch.bfloat16).float()


@pytest.fixture(autouse=True)
def _forget():
    yield
    torch.cuda.synchronize()
    forget_guards()


def assert_variant(sdlib, c):
    """The library runs case ``c`` on the variant the table says, and the properties it exists for hold."""
    rows, split = sdlib.sd_op_gemm_tile_rows(c.M, c.N, c.K), sdlib.sd_op_gemm_splitk(c.M, c.N, c.K, 0)
    d = derive(c, rows, split)
    print(f"[variant] gemm {case_id(c)}: rows {rows} / split {split} / items {d['items']} (grid {d['grid']}), K tiles {d['kts']}")
    assert (rows, split, d["items"]) == (c.rows, c.split, c.items), (rows, split, d["items"])
    assert all(holds(p, d) for p in c.props), [p for p in c.props if not holds(p, d)]


_SHARED = {GEMM_CASES[i] for i in GEMM_PITCHED}          # run twice (plain and pitched): one fp64 reference
_PROBLEMS = {}


def inputs(c):
    g = torch.Generator().manual_seed(c.M * 7 + c.N + c.K1)
    x = r16(torch.randn(c.M, c.K, generator=g))
    w = r16(torch.randn(c.N, c.K, generator=g) / math.sqrt(c.K))
    b = torch.randn(c.N, generator=g) if c.bias else None
    b2 = torch.randn(c.N, generator=g) if c.bias2 else None
    r = r16(torch.randn(c.M, c.N, generator=g)) if c.res else None
    return x, w, b, b2, r


def problem(c):
    """(x, w, bias, bias2, r, ref, bound) of a case on the CPU; the fp64 reference of a case that runs twice is computed once."""
    if c in _PROBLEMS:
        return _PROBLEMS[c]
    ins = inputs(c)
    p = ins + tuple(gemm_bound(*ins))
    if c in _SHARED:
        _PROBLEMS[c] = p
    return p


def launch(sdlib, c, x, w, b, b2, r, pitched=False):
    """One sd_op_gemm launch of the case into a fresh guarded output (pitched: row pitches wider than the rows, the gap
    columns poisoned / holding the sentinel); synchronises and checks every guard."""
    K2 = c.K - c.K1
    ldx, ldx2, ldr, ldc = (c.K1 + 64, K2 + 8, c.N + 8, c.N + 16) if pitched else (c.K1, K2, c.N, c.N)
    x1 = guarded_input(x[:, :c.K1].contiguous(), torch.bfloat16, ld=ldx, label="X")
    x2 = guarded_input(x[:, c.K1:].contiguous(), torch.bfloat16, ld=ldx2, label="X2") if K2 else None
    wd = guarded_input(w, torch.bfloat16, label="W")
    bd = guarded_input(b, label="bias") if b is not None else None
    b2d = guarded_input(b2, label="bias2") if b2 is not None else None
    rd = guarded_input(r, torch.bfloat16, ld=ldr, label="R") if r is not None else None
    out = guarded((c.M, c.N), torch.bfloat16, ld=ldc)
    _lib.check(sdlib.sd_op_gemm(stream(), _lib.ptr(x1), ldx, _lib.ptr(x2), ldx2 if K2 else 0, c.K1, _lib.ptr(wd), _lib.ptr(bd),
                                _lib.ptr(b2d), _lib.ptr(rd), ldr if r is not None else 0, _lib.ptr(out), ldc, c.M, c.N, c.K, 0))
    torch.cuda.synchronize()
    check_guards()
    return out


@pytest.mark.parametrize("c", GEMM_CASES + [FAULT_CASE], ids=case_id)
def test_gemm_splitk(sdlib, c):
    assert_variant(sdlib, c)
    x, w, b, b2, r, ref, bound = problem(c)
    out = launch(sdlib, c, x, w, b, b2, r)
    assert_elementwise(out, ref, bound, f"gemm split-K {case_id(c)} ({c.why})", ("row", "col"))


@pytest.mark.parametrize("c", [GEMM_CASES[i] for i in GEMM_PITCHED], ids=case_id)
def test_gemm_splitk_pitched_operands(sdlib, c):
    """ldx = K1 + 64, ldx2 = K - K1 + 8, ldr = N + 8, ldc = N + 16: the reduce kernel reads R through ldr and stores through
    ldc while the slabs stay N wide; a gap column read turns the output NaN, one written trips its guard."""
    assert_variant(sdlib, c)
    x, w, b, b2, r, ref, bound = problem(c)
    out = launch(sdlib, c, x, w, b, b2, r, pitched=True)
    assert_elementwise(out, ref, bound, f"gemm split-K pitched {case_id(c)}", ("row", "col"))


def test_gemm_splitk_is_run_to_run_deterministic(sdlib):
    """The split-K finish adds the slabs in split order: two launches of the >512-item case agree bit for bit."""
    c = GEMM_CASES[GEMM_DETERMINISM]
    assert_variant(sdlib, c)
    x, w, b, b2, r = inputs(c)
    a = launch(sdlib, c, x, w, b, b2, r)
    bb = launch(sdlib, c, x, w, b, b2, r)
    assert torch.isfinite(a.float()).all()
    assert torch.equal(a, bb), f"{int((a != bb).sum())} of {a.numel()} elements differ between two launches"


@pytest.mark.parametrize("c", CONV_CASES, ids=case_id)
def test_conv3x3_implicit_gemm_splitk(sdlib, c):
    """Stride-2 3x3 convs on the implicit-GEMM kernel (AMODE_CONV) with split-K over many 128-row tiles; the second case has
    more items than workgroups, so the prefetch of a workgroup's next item crosses an image and a split boundary."""
    M, N, K, Ho, Wo = conv_dims(c)
    assert sdlib.sd_op_conv3x3_kernel(M, N, c.Cin, c.H, c.W, c.stride, 0, 0) == 0              # implicit GEMM, not the halo kernel
    split = sdlib.sd_op_conv3x3_splitk(M, N, c.Cin, c.H, c.W, c.stride, 0)
    d = derive(c, 128, split)
    print(f"[variant] {case_id(c)}: rows 128 / split {split} / items {d['items']} (grid {d['grid']}), K tiles {d['kts']}")
    assert (split, d["items"]) == (c.split, c.items), (split, d["items"])
    assert all(holds(p, d) for p in c.props), [p for p in c.props if not holds(p, d)]
    g = torch.Generator().manual_seed(c.B * 100 + c.H + c.Cin)
    x = r16(torch.randn(c.B, c.Cin, c.H, c.W, generator=g))
    w = r16(torch.randn(c.Cout, c.Cin, 3, 3, generator=g) / math.sqrt(K))
    b = torch.randn(c.Cout, generator=g)
    b2 = torch.randn(c.Cout, generator=g) if c.bias2 else None
    r = r16(torch.randn(c.B, c.Cout, Ho, Wo, generator=g)) if c.res else None
    xd = guarded_input(x.permute(0, 2, 3, 1).contiguous(), torch.bfloat16, label="X")
    wd = guarded_input(w.permute(0, 2, 3, 1).reshape(c.Cout, 9, c.Cin // 64, 64).permute(0, 2, 1, 3).contiguous(), torch.bfloat16,
                       label="W")
    bd = guarded_input(b, label="bias")
    b2d = guarded_input(b2, label="bias2") if c.bias2 else None
    rd = guarded_input(r.permute(0, 2, 3, 1).contiguous(), torch.bfloat16, label="R") if c.res else None
    out = guarded((c.B, Ho, Wo, c.Cout), torch.bfloat16)
    _lib.check(sdlib.sd_op_conv3x3(stream(), _lib.ptr(xd), _lib.ptr(wd), _lib.ptr(bd), _lib.ptr(b2d), _lib.ptr(rd), _lib.ptr(out),
                                   c.B, c.H, c.W, c.Cin, c.Cout, c.stride, 0))
    torch.cuda.synchronize()
    check_guards()
    r64, m64 = conv3x3_nhwc_ref(x, w, b, b2, r, c.stride, 0)
    assert_elementwise(out, r64, linear_bound(r64, m64, 9 * c.Cin + 3), f"conv3x3 split-K {case_id(c)} ({c.why})", NHWC)
