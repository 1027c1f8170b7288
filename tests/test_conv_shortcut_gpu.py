"""A ResNet block's conv2 with the 1x1 conv_shortcut folded into the same launch (csrc/conv_halo.hip, SC = 1), through
sd_op_conv3x3_shortcut: per element against the fp64 3x3 conv + fp64 1x1 product of the same bf16-rounded operands, with the
a-priori bound of tests/bounds.py (one output ulp + fp32 summation of 9 Cin + Csc products + the bias); every operand and
output between guard bands.  And the plan: the small UNet built with SD_SHORTCUT_FUSE 0 and 1 against the fp32 oracle."""
import ctypes as C
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

from sonicdiffusionbayeslab_amd import _lib
from tests.bounds import (assert_elementwise, check_guards, conv3x3_nhwc_ref, guarded, guarded_input, linear_bound,
                          norm_ref_bound)
from tests.util import oracle_cfg, rel_l2, synth_inputs

NHWC = ("b", "y", "x", "c")
UNET_TOL = 2e-2             # tests/test_unet_gpu.py's oracle gate


def r16(t):
    return t.to(torch.bfloat16).float()


def stream():
    return torch.cuda.current_stream().cuda_stream


def pack_w(w):
    """[Cout, Cin, 3, 3] -> [Cout][Cin/64][9][64], the conv kernels' K order."""
    Cout, Cin = w.shape[:2]
    return w.permute(0, 2, 3, 1).reshape(Cout, 9, Cin // 64, 64).permute(0, 2, 1, 3).contiguous()


class Case:
    """Operands of one fused launch (host copies rounded to bf16, guarded device copies) and its fp64 reference."""

    def __init__(self, B, H, W, Cin, Cout, Cs1, Cs2):
        g = torch.Generator().manual_seed(B * 1000 + H * 10 + W + Cin + Cout + Cs1 + 3 * Cs2)
        Cs = Cs1 + Cs2
        self.shape = (B, H, W, Cin, Cout, Cs1, Cs2)
        self.x = r16(torch.randn(B, Cin, H, W, generator=g))
        self.w = r16(torch.randn(Cout, Cin, 3, 3, generator=g) / (9 * Cin) ** 0.5)
        self.xs = r16(torch.randn(B, H, W, Cs, generator=g))                 # the shortcut's input, NHWC, [x1 | x2]
        self.wsc = r16(torch.randn(Cout, Cs, generator=g) / Cs ** 0.5)
        self.b = torch.randn(Cout, generator=g)                                # conv2.bias + conv_shortcut.bias
        ref, mag = conv3x3_nhwc_ref(self.x, self.w, self.b)
        self.ref = ref + self.xs.double() @ self.wsc.double().t()
        self.mag = mag + self.xs.double().abs() @ self.wsc.double().abs().t()
        self.bound = linear_bound(self.ref, self.mag, 9 * Cin + Cs + 3)
        bf = torch.bfloat16
        self.xd = guarded_input(self.x.permute(0, 2, 3, 1).contiguous(), bf)
        self.wd = guarded_input(pack_w(self.w), bf)
        self.x1d = guarded_input(self.xs[..., :Cs1].contiguous(), bf)
        self.x2d = guarded_input(self.xs[..., Cs1:].contiguous(), bf) if Cs2 else None
        self.wscd = guarded_input(self.wsc, bf)
        self.bd = guarded_input(self.b)

    def launch(self, sdlib):
        B, H, W, Cin, Cout, Cs1, Cs2 = self.shape
        out = guarded((B, H, W, Cout), torch.bfloat16)
        _lib.check(sdlib.sd_op_conv3x3_shortcut(stream(), self.xd.data_ptr(), self.wd.data_ptr(), self.bd.data_ptr(),
                                                self.x1d.data_ptr(), Cs1, self.x2d.data_ptr() if Cs2 else None, Cs2,
                                                self.wscd.data_ptr(), out.data_ptr(), B, H, W, Cin, Cout))
        return out


# (B, H, W, Cin, Cout, Cs1, Cs2, split-K expected)
CASES = [
    (2, 16, 16, 320, 320, 320, 320, False),     # two segments, 10 shortcut tiles
    (1, 16, 16, 64, 192, 64, 0, False),         # one tile only (prologue meets epilogue), Cout tail in the second channel tile
    (3, 16, 16, 128, 320, 128, 64, False),      # odd tile count, segment switch at an even stage
    (1, 16, 16, 1280, 320, 192, 128, True),     # split-K: 5 tiles over the splits, some splits get none
    (5, 8, 8, 256, 192, 64, 64, False),         # four images per tile plus an M-tail tile
    (2, 14, 18, 128, 192, 64, 128, False),      # geometry mode (tests/test_resolution_edges_gpu.py's smallest halo size): rows beyond mend
]


@pytest.mark.parametrize("B,H,W,Cin,Cout,Cs1,Cs2,split", CASES)
def test_conv3x3_with_folded_shortcut(sdlib, B, H, W, Cin, Cout, Cs1, Cs2, split):
    assert sdlib.sd_op_conv3x3_kernel(B * H * W, Cout, Cin, H, W, 1, 0, 0) == 1          # the halo kernel's 9-tap mode
    splitk = sdlib.sd_op_conv3x3_splitk(B * H * W, Cout, Cin, H, W, 1, 0)
    if split:
        assert splitk > 1 and (Cs1 + Cs2) // 64 % splitk != 0                             # an uneven spread of the shortcut tiles
    c = Case(B, H, W, Cin, Cout, Cs1, Cs2)
    out = c.launch(sdlib)
    torch.cuda.synchronize()
    check_guards()
    print(f"conv3x3+shortcut {B}x{H}x{W} {Cin}->{Cout} Csc={Cs1}+{Cs2}: split-K {splitk} rel-L2 {rel_l2(out, c.ref):.3e}")
    assert_elementwise(out, c.ref, c.bound, f"conv3x3+shortcut {B}x{H}x{W} {Cin}->{Cout} Csc={Cs1}+{Cs2}", NHWC)


def test_folded_shortcut_is_deterministic(sdlib):
    """Six launches into fresh outputs give identical bits (split-K case: fixed-order slab reduction, no atomics)."""
    for shape in [(1, 16, 16, 1280, 320, 192, 128), (3, 16, 16, 128, 320, 128, 64)]:
        c = Case(*shape)
        outs = [c.launch(sdlib) for _ in range(6)]
        torch.cuda.synchronize()
        check_guards()
        assert torch.isfinite(outs[0]).all()
        for o in outs[1:]:
            assert torch.equal(o.view(torch.int16), outs[0].view(torch.int16))


def test_shape_the_halo_kernel_does_not_take_is_an_error(sdlib):
    """Stride-1 convs of 4x4 images run on the implicit-GEMM kernel, which has no shortcut phase: an error code, no launch."""
    c = Case(2, 4, 4, 64, 160, 64, 0)
    assert sdlib.sd_op_conv3x3_kernel(2 * 16, 160, 64, 4, 4, 1, 0, 0) == 0
    out = guarded((2, 4, 4, 160), torch.bfloat16, fill=0.0)
    rc = sdlib.sd_op_conv3x3_shortcut(stream(), c.xd.data_ptr(), c.wd.data_ptr(), c.bd.data_ptr(), c.x1d.data_ptr(), 64, None, 0,
                                      c.wscd.data_ptr(), out.data_ptr(), 2, 4, 4, 64, 160)
    assert rc != 0 and b"shortcut" in sdlib.sd_last_error()
    rc = sdlib.sd_op_conv3x3_shortcut(stream(), c.xd.data_ptr(), c.wd.data_ptr(), c.bd.data_ptr(), c.x1d.data_ptr(), 32, None, 0,
                                      c.wscd.data_ptr(), out.data_ptr(), 2, 16, 16, 64, 160)       # half a K tile
    assert rc != 0
    torch.cuda.synchronize()
    assert (out == 0).all()
    check_guards()


@pytest.mark.parametrize("B,H,Cin,Cout,Cs1,Cs2", [(1, 32, 64, 256, 64, 64), (2, 64, 128, 320, 192, 0)])
def test_folded_shortcut_groupnorm_producer_statistics(sdlib, B, H, Cin, Cout, Cs1, Cs2):
    """The GroupNorm block statistics of a fused launch are those of its own stored output: the GroupNorm fed from the
    epilogue's statistics against the same GroupNorm computing them from the stored tensor, and both against fp64 from the
    stored values (the check of test_ops_gpu.py::test_conv3x3_groupnorm_producer_statistics)."""
    c = Case(B, H, H, Cin, Cout, Cs1, Cs2)
    g = torch.Generator().manual_seed(H + Cout)
    gamma, beta = torch.randn(Cout, generator=g), torch.randn(Cout, generator=g)
    gd, btd = guarded_input(gamma), guarded_input(beta)
    y, yn, own = (guarded((B, H, H, Cout), torch.bfloat16) for _ in range(3))
    _lib.check(sdlib.sd_op_conv3x3_shortcut_groupnorm(stream(), c.xd.data_ptr(), c.wd.data_ptr(), c.bd.data_ptr(), c.x1d.data_ptr(),
                                                      Cs1, c.x2d.data_ptr() if Cs2 else None, Cs2, c.wscd.data_ptr(), y.data_ptr(),
                                                      B, H, H, Cin, Cout, gd.data_ptr(), btd.data_ptr(), yn.data_ptr(), 32, 1e-5, 1))
    _lib.check(sdlib.sd_op_groupnorm(stream(), y.data_ptr(), Cout, None, 0, gd.data_ptr(), btd.data_ptr(), own.data_ptr(), B, H * H,
                                     32, 1e-5, 1))
    torch.cuda.synchronize()
    check_guards()
    assert_elementwise(y, c.ref, c.bound, f"conv3x3+shortcut (+stats) {B}x{H}x{H} {Cin}->{Cout}", NHWC)
    assert rel_l2(yn, own) < 2e-3
    yk = y.float().cpu().view(B, H * H, Cout)
    n64, nb = norm_ref_bound(yk, gamma, beta, H * H * Cout // 32, 1e-5, True, groups=32)
    for i, t in enumerate((yn, own)):
        assert_elementwise(t.view(B, H * H, Cout), n64, nb, f"conv3x3+shortcut groupnorm[{i}]", ("b", "pixel", "c"))


# ---------------------------------------------------------------------------------------------------------------------
# the plan
# ---------------------------------------------------------------------------------------------------------------------

def _op_table(net, lat, ub, cache_mode=0):
    out = torch.empty(ub, 4, lat.shape[2], lat.shape[3], device="cuda")
    ws = net._workspace(ub)
    buf = C.create_string_buffer(1 << 20)
    n = net._lib.sd_unet_forward_op_times(net._handle, _lib.current_stream(), lat.data_ptr(), lat.shape[0], ub, 501.0, out.data_ptr(),
                                          net._ws_ptr(ws), ws.numel() - 256, cache_mode, net.cache_branch_id, buf, len(buf))
    assert n > 0
    return [[float(v) for v in l.split()] for l in buf.value.decode().splitlines()]


def _shortcut_gemms(rows):
    """conv_shortcut GEMMs of an op table: a GEMM (kind 5) whose output is the residual of the 3x3 conv (kind 4) launched
    right after it -- same M and N, the conv's K = 9 N (a resnet's conv2).  Returns each one's (M, N) as integers."""
    return [(int(b[2]), int(b[3])) for a, b in zip(rows, rows[1:])
            if int(a[1]) == 5 and int(b[1]) == 4 and a[2] == b[2] and a[3] == b[3] and b[4] == 9 * b[3]]


def _on_halo_kernel(sdlib, M, N, ub):
    """Whether the resnet conv2 [M, N] of a square level at UNet batch ub runs on the halo kernel (which has the shortcut phase)."""
    side = int(round((M // ub) ** 0.5))
    assert side * side * ub == M
    return sdlib.sd_op_conv3x3_kernel(M, N, N, side, side, 1, 0, 0) == 1


def _fused_convs(rows):
    """conv2 launches that carry a shortcut: the reported work exceeds the 3x3 conv's 2 M N K flops."""
    return sum(int(r[1]) == 4 and r[6] * 1e9 > 2.0 * r[2] * r[3] * r[4] * 1.001 for r in rows)


@pytest.fixture(scope="module")
def plans():
    """The small UNet of tests/test_unet_gpu.py twice in one process: SD_SHORTCUT_FUSE=0 (the separate GEMM) and the default."""
    from oracle.unet import unet_forward
    from sonicdiffusionbayeslab_amd.unet import HipUNet2DConditionModel
    from sonicdiffusionbayeslab_amd.weights import UNetConfig, make_synthetic_state_dict
    cfg = UNetConfig(sample_size=16)
    sd = make_synthetic_state_dict(cfg, seed=1234)
    old = os.environ.get("SD_SHORTCUT_FUSE")
    nets = {}
    try:
        for fuse in ("0", "1"):
            os.environ["SD_SHORTCUT_FUSE"] = fuse
            nets[fuse] = HipUNet2DConditionModel(cfg, sd)
            # a plan is built when it is first asked for: do that while the switch is set
            lat, pe, ne = synth_inputs(cfg, 1)
            for branch in (-1, 1):
                nets[fuse].set_deepcache(branch)
                nets[fuse].set_context(torch.cat([ne, pe]).cuda())
            nets[fuse].set_deepcache(-1)
    finally:
        if old is None:
            os.environ.pop("SD_SHORTCUT_FUSE", None)
        else:
            os.environ["SD_SHORTCUT_FUSE"] = old
    lat, pe, ne = synth_inputs(cfg, 1)
    ctx = torch.cat([ne, pe])
    with torch.no_grad():
        ref = unet_forward(sd, oracle_cfg(cfg), torch.cat([lat, lat]), 501.0, ctx)
    return cfg, nets, lat, ctx, ref


@pytest.mark.parametrize("fuse", ["0", "1"])
def test_cfg_pair_plan_matches_oracle_with_and_without_the_fusion(sdlib, plans, fuse):
    cfg, nets, lat, ctx, ref = plans
    net = nets[fuse]
    net.set_deepcache(-1)
    net.set_context(ctx.cuda())
    eps = net.forward_latents(lat.cuda(), 2, 501.0)            # latent batch 1 -> UNet batch 2: the CFG-pair plan
    torch.cuda.synchronize()
    err = rel_l2(eps, ref)
    rows = _op_table(net, lat.cuda(), 2)
    print(f"SD_SHORTCUT_FUSE={fuse}: rel-L2 vs oracle {err:.3e}; shortcut GEMMs {len(_shortcut_gemms(rows))}, fused convs {_fused_convs(rows)}")
    assert torch.isfinite(eps).all() and err < UNET_TOL
    # The small UNet has the SD-1.5 block layout: 14 resnets change their channel count (up_blocks.0-3 x 3, down_blocks.1 / 2
    # resnets.0).  Its 16x16 and 8x8 levels run conv2 on the halo kernel (3 + 4 resnets); its 4x4 and 2x2 levels are below the
    # halo kernel's smallest width and keep the GEMM (4 + 3).
    gemms = _shortcut_gemms(rows)
    halo = [_on_halo_kernel(sdlib, M, N, 2) for M, N in gemms]
    if fuse == "1":
        assert not any(halo), gemms                   # no conv_shortcut GEMM wherever conv2 could carry it
        assert _fused_convs(rows) == 7 and len(gemms) == 7
    else:
        assert len(gemms) == 14 and sum(halo) == 7 and _fused_convs(rows) == 0


@pytest.mark.parametrize("fuse", ["0", "1"])
def test_deepcache_plan_matches_oracle_with_and_without_the_fusion(sdlib, plans, fuse):
    """A DeepCache plan: the full step that stores the cached features, then a skip step on the same inputs, which must
    reproduce it from the cache -- both against the oracle."""
    from sonicdiffusionbayeslab_amd.unet import CACHE_FULL_AND_STORE, CACHE_SKIP
    cfg, nets, lat, ctx, ref = plans
    net = nets[fuse]
    net.set_deepcache(1)
    try:
        net.set_context(ctx.cuda())
        full = net.forward_latents(lat.cuda(), 2, 501.0, cache_mode=CACHE_FULL_AND_STORE).clone()
        skip = net.forward_latents(lat.cuda(), 2, 501.0, cache_mode=CACHE_SKIP).clone()
        torch.cuda.synchronize()
        rows = _op_table(net, lat.cuda(), 2, CACHE_FULL_AND_STORE)
    finally:
        net.set_deepcache(-1)
    print(f"SD_SHORTCUT_FUSE={fuse} DeepCache: full {rel_l2(full, ref):.3e} skip {rel_l2(skip, ref):.3e}")
    assert torch.isfinite(full).all() and rel_l2(full, ref) < UNET_TOL
    assert torch.isfinite(skip).all() and rel_l2(skip, ref) < UNET_TOL
    on_halo = sum(_on_halo_kernel(sdlib, M, N, 2) for M, N in _shortcut_gemms(rows))
    assert on_halo == (0 if fuse == "1" else 7) and _fused_convs(rows) == (7 if fuse == "1" else 0)
