"""GPU parity of the tiny autoencoder (AutoencoderTiny / TAESD): the 64-channel conv kernel, the entry and the exit kernel per
element against fp64 with a-priori bounds and guard bands, both halves against the fp32 oracle (tests/taesd_oracle.py) at a
gate measured from the oracle's own bf16 emulation, batch / order independence bit for bit, and the pipeline wiring.

The measured figures are in profiles/taesd_notes.md."""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from sonicdiffusionbayeslab_amd import _lib
from tests.bounds import (ATOL_TINY, U32, assert_elementwise, check_guards, conv3x3_nhwc_ref, forget_guards, guarded,
                          guarded_input, linear_bound, ulp_fp32)
from tests.util import cosine, oracle_cfg, rel_l2, synth_inputs

NHWC = ("b", "y", "x", "c")
NCHW = ("b", "c", "y", "x")
ENC_TOL, ENC_COS = 2e-2, 0.999            # tests/test_img2img_gpu.py: the start latents of an image-to-image loop
FREE_TOL, FREE_COS = 6e-2, 0.998          # ... and its free-running final latents


def stream():
    return torch.cuda.current_stream().cuda_stream


@pytest.fixture(autouse=True)
def _drop_guards():
    yield
    torch.cuda.synchronize()
    forget_guards()


def r16(t):
    return t.to(torch.bfloat16).float()


# ---------------------------------------------------------------- sd_op_conv64 per element
# csrc/conv64.hip: output tiles of 8 rows x 32 columns (modes 0 and 1; mode 1's halo is 6 x 18 low-res pixels) and of 4 rows x
# 16 columns (mode 2); one workgroup takes tiles t, t + grid, ...  The shapes below, against those constants:
#   8x8      smaller than a tile in both directions
#   24x40 B2 ragged right tile (40 = 32 + 8), three tile rows, two samples: a halo must not read the neighbouring sample
#   20x70    3 x 3 tiles with ragged right and bottom tiles: the centre tile has halos on four sides
#   8x520    17 tiles wide: more halo slots per image row than the halo kernel's 400-slot rule allows
#   mode 1:  12x20 -> 24x40 (B 2) and 10x50 -> 20x100 (3 x 4 tiles)
#   mode 2:  16x24 -> 8x12, 8x8 -> 4x4, 26x100 -> 13x50 (4 x 4 tiles, ragged) and the odd 9x35 -> 5x18 (B 2)
CONV64_CASES = [
    # name, B, Hin, Win, mode, bias, residual, relu
    ("plain+b+relu 8x8", 1, 8, 8, 0, True, False, True),
    ("plain+b+R+relu 24x40", 2, 24, 40, 0, True, True, True),
    ("plain+b+R+relu 20x70", 1, 20, 70, 0, True, True, True),
    ("plain+b+relu 20x70", 2, 20, 70, 0, True, False, True),
    ("plain+b+relu 8x520", 1, 8, 520, 0, True, False, True),
    ("up 12x20", 2, 12, 20, 1, False, False, False),
    ("up 10x50", 1, 10, 50, 1, False, False, False),
    ("s2 16x24", 1, 16, 24, 2, False, False, False),
    ("s2 8x8", 2, 8, 8, 2, False, False, False),
    ("s2 26x100", 1, 26, 100, 2, False, False, False),
    ("s2 9x35", 2, 9, 35, 2, False, False, False),
]

# Past one round.  The grid is min(ntiles, 256) and every case above has at most 18 tiles: no workgroup there takes a second
# tile, so neither the prefetch into the other halo buffer nor the buffer flip is exercised.  The cases below have 2 x 19 x 14
# = 532 tiles each: work indices 0 .. 19 run three rounds (the third is the first that reads a halo buffer after a refill),
# the others two (the `t + nblk < ntiles` guard decides), the sample boundary falls at tile 266 in the middle of round 2, and
# the bottom and right tiles are ragged (150 = 18 x 8 + 6, 420 = 13 x 32 + 4; mode 2: 75 = 18 x 4 + 3, 210 = 13 x 16 + 2).
CONV64_THREE_ROUNDS = [
    ("plain+b+R+relu 150x420 3 rounds", 2, 150, 420, 0, True, True, True),
    ("plain+b+relu 150x420 3 rounds", 2, 150, 420, 0, True, False, True),
    ("up 75x210 3 rounds", 2, 75, 210, 1, False, False, False),
    ("s2 149x419 3 rounds", 2, 149, 419, 2, False, False, False),
]
CONV64_CASES += CONV64_THREE_ROUNDS
CONV64_GRID_CAP = 256


def _conv64_out(n, mode):
    return 2 * n if mode == 1 else (n - 1) // 2 + 1 if mode == 2 else n


def _conv64_ntiles(B, Hin, Win, mode):
    """The tile count of csrc/conv64.hip restated: output tiles of 8 rows x 32 columns (modes 0 and 1) or 4 x 16 (mode 2)."""
    tr, tc = (4, 16) if mode == 2 else (8, 32)
    return B * (-(-_conv64_out(Hin, mode) // tr)) * (-(-_conv64_out(Win, mode) // tc))


def _pack64(sdlib, w):
    n = sdlib.sd_op_conv64_pack(None, None)
    assert n == 9 * 64 * 64 * 2
    out = torch.empty(n // 2, dtype=torch.int16)
    wc = w.float().contiguous()
    assert sdlib.sd_op_conv64_pack(wc.data_ptr(), out.data_ptr()) == n
    return out.view(torch.bfloat16)


@pytest.mark.parametrize("name,B,H,W,mode,has_b,has_r,relu", CONV64_CASES, ids=[c[0] for c in CONV64_CASES])
def test_conv64_per_element(sdlib, name, B, H, W, mode, has_b, has_r, relu):
    if any(name == c[0] for c in CONV64_THREE_ROUNDS):
        ntiles = _conv64_ntiles(B, H, W, mode)
        assert ntiles > 2 * CONV64_GRID_CAP, ntiles              # some workgroups run three rounds ...
        assert ntiles % CONV64_GRID_CAP != 0, ntiles             # ... and the others one fewer: the prefetch guard matters
    g = torch.Generator().manual_seed(1000 * mode + H * W + B)
    x = r16(torch.randn(B, 64, H, W, generator=g))
    w = r16(torch.randn(64, 64, 3, 3, generator=g) / math.sqrt(576))
    b = 0.1 * torch.randn(64, generator=g) if has_b else None
    Ho, Wo = (2 * H, 2 * W) if mode == 1 else ((H - 1) // 2 + 1, (W - 1) // 2 + 1) if mode == 2 else (H, W)
    r = r16(torch.randn(B, 64, Ho, Wo, generator=g)) if has_r else None
    xd = guarded_input(x.permute(0, 2, 3, 1).contiguous(), torch.bfloat16)
    wd = guarded_input(_pack64(sdlib, w), torch.bfloat16)
    bd = guarded_input(b) if has_b else None
    rd = guarded_input(r.permute(0, 2, 3, 1).contiguous(), torch.bfloat16) if has_r else None
    out = guarded((B, Ho, Wo, 64), torch.bfloat16)
    _lib.check(sdlib.sd_op_conv64(stream(), xd.data_ptr(), wd.data_ptr(), _lib.ptr(bd), _lib.ptr(rd), out.data_ptr(), B, H, W, mode,
                                  1 if relu else 0))
    torch.cuda.synchronize()
    check_guards()
    ref, mag = conv3x3_nhwc_ref(x, w, b, None, r, stride=2 if mode == 2 else 1, up=1 if mode == 1 else 0)
    assert ref.shape == (B, Ho, Wo, 64)
    if relu:
        clipped = float((ref <= 0).double().mean())
        assert 0.35 < clipped < 0.65, clipped                    # the ReLU matters: about half the outputs are clipped
        ref = ref.clamp(min=0.0)
    print(f"conv64 {name}: rel-L2 {rel_l2(out, ref):.3e}")
    assert_elementwise(out, ref, linear_bound(ref, mag, 576), f"conv64 {name}", NHWC)


def test_conv64_refuses_bad_arguments(sdlib):
    x = torch.zeros(1, 8, 8, 64, dtype=torch.bfloat16, device="cuda")
    w = torch.zeros(9 * 64 * 64, dtype=torch.bfloat16, device="cuda")
    y = torch.zeros_like(x)
    assert sdlib.sd_op_conv64(stream(), x.data_ptr(), w.data_ptr(), None, None, y.data_ptr(), 1, 8, 8, 3, 0) != 0
    assert sdlib.sd_op_conv64(stream(), x.data_ptr(), w.data_ptr(), None, None, x.data_ptr(), 1, 8, 8, 0, 0) != 0     # in place
    assert sdlib.sd_op_conv64(stream(), x.data_ptr(), w.data_ptr(), None, None, y.data_ptr(), 0, 8, 8, 0, 0) != 0
    assert sdlib.sd_op_conv64(stream(), x.data_ptr(), None, None, None, y.data_ptr(), 1, 8, 8, 0, 0) != 0
    # 31 x 1024 x 1024 pixels x 128 bytes = 4.16e9 > 0xf0000000: past the 32-bit DMA offsets, refused before any launch
    assert sdlib.sd_op_conv64(stream(), x.data_ptr(), w.data_ptr(), None, None, y.data_ptr(), 31, 1024, 1024, 0, 0) != 0
    msg = sdlib.sd_last_error().decode()
    assert str(31 * 1024 * 1024 * 128) in msg and str(0xf0000000) in msg, msg


# ---------------------------------------------------------------- sd_op_conv64 with DMA offsets at and above 2^31
def _conv64_crop_check(what, xs, ys, w, b, relu, mode, oy0, oy1, ox0, ox1):
    """Outputs [oy0, oy1) x [ox0, ox1) of one sample per element on the host: xs [H, W, 64] and ys [Ho, Wo, 64] stay on the
    device, only the input window with its one-pixel rim and the output window come back.  The reference pads the window
    with zeros, which is the image's padding only where the window ends at the image's edge: an output is compared if every
    row and column of its 3x3 support lies inside the window or outside the image."""
    H, W = xs.shape[:2]
    st = 2 if mode == 2 else 1

    def window(o0, o1, n):
        i0 = max(st * o0 - st, 0)                                 # (a multiple of the stride: reference row r is output i0 / st + r)
        i1 = min(st * (o1 - 1) + 2, n)
        r = torch.arange((i1 - i0 - 1) // st + 1)
        ok = ((st * r - 1 >= 0) | (i0 == 0)) & ((st * r + 1 <= i1 - i0 - 1) | (i1 == n))
        return i0, i1, i0 // st, ok

    iy0, iy1, ry0, oky = window(oy0, oy1, H)
    ix0, ix1, rx0, okx = window(ox0, ox1, W)
    ref, mag = conv3x3_nhwc_ref(xs[iy0:iy1, ix0:ix1].float().cpu().permute(2, 0, 1)[None], w, b, stride=st)
    got = ys[ry0:ry0 + ref.shape[1], rx0:rx0 + ref.shape[2]].float().cpu()[None]
    assert got.shape == ref.shape, (got.shape, ref.shape)
    rows, cols = torch.nonzero(oky).flatten() + ry0, torch.nonzero(okx).flatten() + rx0
    assert set(range(oy0, oy1)) <= set(rows.tolist()) and set(range(ox0, ox1)) <= set(cols.tolist())
    ref, mag, got = (t[:, oky][:, :, okx] for t in (ref, mag, got))
    if relu:
        clipped = float((ref <= 0).double().mean())
        assert 0.35 < clipped < 0.65, clipped
        ref = ref.clamp(min=0.0)
    print(f"conv64 {what} rows {int(rows[0])}..{int(rows[-1])} cols {int(cols[0])}..{int(cols[-1])}: rel-L2 {rel_l2(got, ref):.3e}")
    assert_elementwise(got, ref, linear_bound(ref, mag, 576), f"conv64 {what}", NHWC)


def test_conv64_offsets_past_2g(sdlib):
    """A halo's source offset is a 32-bit byte offset into the input.  17 images of 1024 x 1024 pixels are 2.28e9 bytes and
    sample 16 starts at byte 2^31 exactly: every offset of that sample has its top bit set.  Samples 0, 15 and 16 alone (all
    offsets below 2^27, the arithmetic test_conv64_per_element checks) must give their slices of the batched output bit for
    bit; three windows of sample 16 are checked per element on the host.  Nothing of full size leaves the device."""
    B, S = 17, 1024
    assert (B - 1) * S * S * 128 == 2 ** 31 and B * S * S * 128 <= 0xf0000000
    g = torch.Generator().manual_seed(2031)
    w = r16(torch.randn(64, 64, 3, 3, generator=g) / math.sqrt(576))
    b = 0.1 * torch.randn(64, generator=g)
    x = torch.randn(B, S, S, 64, device="cuda", dtype=torch.bfloat16, generator=torch.Generator(device="cuda").manual_seed(2031))
    xd = guarded_input(x, torch.bfloat16)
    del x
    wd, bd = guarded_input(_pack64(sdlib, w), torch.bfloat16), guarded_input(b)
    # mode 0 with bias and ReLU, mode 2 with no epilogue
    for mode, relu in ((0, True), (2, False)):
        So = _conv64_out(S, mode)
        out = guarded((B, So, So, 64), torch.bfloat16)
        _lib.check(sdlib.sd_op_conv64(stream(), xd.data_ptr(), wd.data_ptr(), _lib.ptr(bd if relu else None), None, out.data_ptr(),
                                      B, S, S, mode, 1 if relu else 0))
        torch.cuda.synchronize()
        assert not bool(torch.isnan(out).any()), f"mode {mode}: NaN left in the output"
        for s in (0, 15, 16):
            one = guarded((1, So, So, 64), torch.bfloat16)
            _lib.check(sdlib.sd_op_conv64(stream(), xd[s:s + 1].data_ptr(), wd.data_ptr(), _lib.ptr(bd if relu else None), None,
                                          one.data_ptr(), 1, S, S, mode, 1 if relu else 0))
            torch.cuda.synchronize()
            assert torch.equal(one, out[s:s + 1]), f"mode {mode}: sample {s} alone differs from its slice of the batch"
        # the top-left and bottom-right corners of the image and a window across the tile corner at the output's centre
        # (a multiple of 8 x 32 and of 4 x 16)
        c = So // 2
        for tag, (oy0, ox0) in (("top left", (0, 0)), ("bottom right", (So - 24, So - 48)), ("tile corner", (c - 12, c - 24))):
            _conv64_crop_check(f"mode {mode} past 2^31, {tag}", xd[16], out[16], w, b if relu else None, relu, mode,
                               oy0, oy0 + 24, ox0, ox0 + 48)
    check_guards()


# ---------------------------------------------------------------- entry and exit kernels per element
@pytest.mark.parametrize("B,H,W", [(1, 8, 8), (2, 24, 40)])
@pytest.mark.parametrize("decoder", [True, False])
def test_entry_kernel_per_element(sdlib, B, H, W, decoder):
    """fp32 conv on the fp32 input.  Decoder: the input is tanh(z / 3) * 3 evaluated in fp32 -- the constant 1/3, the
    product, tanhf (<= 2 ulp) and the final product carry at most (1 + 1 + 4 + 1) u = 7 u of relative error into each input
    (d tanh(y) / dy * y / tanh(y) <= 1), i.e. 7 u mag into the sum: k_eff = 9 Cin products + the bias + 7."""
    cin = 4 if decoder else 3
    g = torch.Generator().manual_seed(H * W + cin)
    x = torch.randn(B, cin, H, W, generator=g) * 2.5 if decoder else torch.rand(B, cin, H, W, generator=g)
    w = torch.randn(64, cin, 3, 3, generator=g) * math.sqrt(2.0 / (9 * cin))
    b = 0.05 * torch.randn(64, generator=g)
    wt = w.permute(1, 2, 3, 0).reshape(cin * 9, 64).contiguous()          # [Cin * 9][64]
    xd, wd, bd = guarded_input(x), guarded_input(wt), guarded_input(b)
    out = guarded((B, H, W, 64), torch.bfloat16)
    _lib.check(sdlib.sd_op_taesd_entry(stream(), xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), out.data_ptr(), B, H, W, cin,
                                       1 if decoder else 0))
    torch.cuda.synchronize()
    check_guards()
    xin = torch.tanh(x.double() / 3) * 3 if decoder else x.double()
    ref, mag = conv3x3_nhwc_ref(xin, w, b)
    if decoder:
        ref = ref.clamp(min=0.0)
    assert_elementwise(out, ref, linear_bound(ref, mag, 9 * cin + 1 + (7 if decoder else 0)),
                       f"taesd entry {'decoder' if decoder else 'encoder'} {B}x{H}x{W}", NHWC)


@pytest.mark.parametrize("B,H,W", [(1, 8, 8), (2, 24, 40)])
@pytest.mark.parametrize("cout", [3, 4])
def test_exit_kernel_per_element(sdlib, B, H, W, cout):
    g = torch.Generator().manual_seed(H * W + cout)
    x = r16(torch.randn(B, 64, H, W, generator=g).abs())                  # post-ReLU activations
    w = r16(torch.randn(cout, 64, 3, 3, generator=g) / math.sqrt(576) * 0.5)
    b = 0.5 + 0.05 * torch.randn(cout, generator=g)
    xd = guarded_input(x.permute(0, 2, 3, 1).contiguous(), torch.bfloat16)
    wd = guarded_input(w.permute(0, 2, 3, 1).reshape(cout, 9, 64).contiguous(), torch.bfloat16)      # [Cout][tap][64]
    bd = guarded_input(b)
    outs = {}
    for mode in (0, 1, 2):
        outs[mode] = guarded((B, cout, H, W), torch.float32)
        _lib.check(sdlib.sd_op_taesd_exit(stream(), xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), outs[mode].data_ptr(), B, H, W,
                                          cout, mode))
    torch.cuda.synchronize()
    check_guards()
    y, mag = conv3x3_nhwc_ref(x, w, b)
    y, mag = y.permute(0, 3, 1, 2), mag.permute(0, 3, 1, 2)
    by = linear_bound(y, mag, 577, out=torch.float32)                     # 576 products + the bias, fp32 output
    assert 0.05 < float(((y < 0) | (y > 1)).double().mean()) < 0.6        # the clamp has something to do (y ~ N(0.5, 0.5))
    assert_elementwise(outs[2], y, by, f"taesd exit raw {cout}ch {B}x{H}x{W}", NCHW)
    ref0 = y * 2 - 1
    assert_elementwise(outs[0], ref0, 2 * by + ulp_fp32(ref0) + ATOL_TINY, f"taesd exit y*2-1 {cout}ch {B}x{H}x{W}", NCHW)
    assert_elementwise(outs[1], y.clamp(0, 1), by, f"taesd exit clamp {cout}ch {B}x{H}x{W}", NCHW)
    # the unit-range mode is what the pipeline's two passes make of the [-1, 1] mode
    two_pass = (outs[0] / 2 + 0.5).clamp(0, 1)
    d = float((outs[1] - two_pass).abs().max())
    print(f"taesd exit {cout}ch {B}x{H}x{W}: unit_range vs clamp(x / 2 + 0.5) max abs diff {d:.3e}")
    assert d <= 2.0 ** -22


# ---------------------------------------------------------------- both halves against the oracle
@pytest.fixture(scope="module")
def tiny():
    from sonicdiffusionbayeslab_amd.vae import HipTinyVaeDecoder, HipTinyVaeEncoder, make_synthetic_tiny_vae_state_dict
    from tests import taesd_oracle as O
    sd = make_synthetic_tiny_vae_state_dict()
    return sd, O.build(sd), HipTinyVaeDecoder(sd), HipTinyVaeEncoder(sd)


def _image(b, h, w, seed):
    """A smooth picture plus texture in [0, 1] (tests/test_img2img_gpu.py)."""
    g = torch.Generator().manual_seed(seed)
    low = F.interpolate(torch.rand(b, 3, max(h // 16, 2), max(w // 16, 2), generator=g), size=(h, w), mode="bilinear", align_corners=False)
    return (0.8 * low + 0.2 * torch.rand(b, 3, h, w, generator=g)).clamp(0, 1)


def _gate(what, got, ref32, ref_bf16):
    """rel-L2(hip, fp32 oracle) <= 2 x floor, floor = rel-L2(the oracle's bf16 emulation, fp32 oracle): the kernel's own
    rounding flips are a second noise sample of the size of the emulation's."""
    floor = rel_l2(ref_bf16, ref32)
    e, c = rel_l2(got, ref32), cosine(got, ref32)
    print(f"taesd {what}: rel-L2 vs fp32 oracle {e:.3e} (floor {floor:.3e}, vs the bf16 emulation {rel_l2(got, ref_bf16):.3e}) cos {c:.6f}")
    assert torch.isfinite(got).all()
    assert e <= 2 * floor and c > 0.999, (what, e, floor, c)


@pytest.mark.parametrize("shape,seed", [((2, 4, 8, 8), 5), ((2, 4, 16, 24), 6), ((1, 4, 64, 64), 11)])      # (512 pixels: 4 rounds)
def test_decoder_matches_oracle(tiny, shape, seed):
    sd, oracle, dec, _ = tiny
    z = torch.randn(shape, generator=torch.Generator().manual_seed(seed))
    got = dec.decode(z.cuda())
    torch.cuda.synchronize()
    assert got.shape == (shape[0], 3, 8 * shape[2], 8 * shape[3]) and got.dtype == torch.float32
    _gate(f"decode {shape}", got, oracle.decode(z), oracle.decode(z, emulate_bf16=True))
    unit = dec.decode(z.cuda(), unit_range=True)
    assert float(unit.min()) >= 0.0 and float(unit.max()) <= 1.0
    assert float((unit - (got / 2 + 0.5).clamp(0, 1)).abs().max()) <= 2.0 ** -22


@pytest.mark.parametrize("shape,seed", [((2, 3, 64, 64), 7), ((2, 3, 128, 192), 8), ((1, 3, 512, 512), 12)])
def test_encoder_matches_oracle(tiny, shape, seed):
    sd, oracle, _, enc = tiny
    img = _image(shape[0], shape[2], shape[3], seed)
    got = enc.encode(img.cuda())
    torch.cuda.synchronize()
    assert got.shape == (shape[0], 4, shape[2] // 8, shape[3] // 8) and got.dtype == torch.float32
    _gate(f"encode {shape}", got, oracle.encode01(img), oracle.encode01(img, emulate_bf16=True))


def test_sizes_outside_the_rule_are_refused(tiny):
    _, _, dec, enc = tiny
    with pytest.raises(ValueError):
        dec.decode(torch.zeros(1, 4, 12, 16))
    with pytest.raises(ValueError):
        dec.decode(torch.zeros(1, 3, 16, 16))
    with pytest.raises(ValueError):
        enc.encode(torch.zeros(1, 3, 100, 128))


def test_batch_and_order_independence(tiny):
    """No split-K, no atomics, and no dependence on which workgroup takes a tile: sample 1 alone is its slice of the batched
    call, and two runs agree, bit for bit."""
    _, _, dec, enc = tiny
    z = torch.randn((3, 4, 16, 24), generator=torch.Generator().manual_seed(9)).cuda()
    a = dec.decode(z)
    assert torch.equal(a, dec.decode(z))
    assert torch.equal(dec.decode(z[1:2]), a[1:2])
    assert torch.equal(dec.decode(z, chunk=2), a)
    img = _image(3, 128, 192, 10).cuda()
    e = enc.encode(img)
    assert torch.equal(e, enc.encode(img))
    assert torch.equal(enc.encode(img[1:2]), e[1:2])
    assert torch.equal(enc.encode(img, chunk=1), e)
    # three full rounds against one: 256 top-level tiles per image, so a B = 1 call never loops and the B = 3 call takes every
    # workgroup through the work loop exactly three times
    z = torch.randn((3, 4, 32, 32), generator=torch.Generator().manual_seed(13)).cuda()
    a = dec.decode(z)
    img = _image(3, 256, 256, 14).cuda()
    e = enc.encode(img)
    for i in range(3):
        assert torch.equal(dec.decode(z[i:i + 1]), a[i:i + 1]), i
        assert torch.equal(enc.encode(img[i:i + 1]), e[i:i + 1]), i


# ---------------------------------------------------------------- pipeline
@pytest.fixture(scope="module")
def env():
    from sonicdiffusionbayeslab_amd.models import StableDiffusionModel
    from sonicdiffusionbayeslab_amd.registry import schedulers_registry
    from sonicdiffusionbayeslab_amd.weights import UNetConfig, make_synthetic_state_dict
    cfg = UNetConfig(sample_size=16)
    sd = make_synthetic_state_dict(cfg, seed=1234)
    model = StableDiffusionModel(unet_config=cfg, state_dict=dict(sd)).to("cuda:0")
    model.scheduler = schedulers_registry["ddim_scheduler"].from_config(model.scheduler.config)
    return cfg, sd, model


def _call(model, cfg, output_type, seed=71):
    lat, pe, ne = synth_inputs(cfg, 2, seed=seed)
    return model(prompt_embeds=pe, negative_prompt_embeds=ne, latents=lat, num_inference_steps=2, guidance_scale=7.5,
                 output_type=output_type, collect_x0=True)


def test_pipeline_all_previews_and_unload(env):
    cfg, sd, model = env
    assert model.tiny_vae_use is None
    before, _, before_x0 = _call(model, cfg, "pt")
    lat, _, lat_x0 = _call(model, cfg, "latent")
    assert len(lat_x0) == 2

    model.load_tiny_vae("madebyollin/taesd", use_for="all")
    try:
        out, _, x0 = _call(model, cfg, "pt")
        tiny = model.tiny_vae_decoder
        assert tiny is not None and len(x0) == 2                           # one preview per step
        assert out.images.shape == (2, 3, 128, 128)
        assert torch.equal(out.images, tiny.decode(lat.images, unit_range=True))
        for p, l in zip(x0, lat_x0):
            assert torch.equal(p, tiny.decode(l, unit_range=True))
        for t in [out.images] + list(x0):
            assert float(t.min()) >= 0.0 and float(t.max()) <= 1.0
        assert not torch.equal(out.images, before.images)
    finally:
        model.unload_tiny_vae()

    model.load_tiny_vae("madebyollin/taesd", use_for="previews")
    try:
        out, _, x0 = _call(model, cfg, "pt")
        assert torch.equal(out.images, before.images)                      # the final image stays on the AutoencoderKL
        for p, l in zip(x0, lat_x0):
            assert torch.equal(p, model.tiny_vae_decoder.decode(l, unit_range=True))
    finally:
        model.unload_tiny_vae()

    after, _, after_x0 = _call(model, cfg, "pt")
    assert torch.equal(after.images, before.images)
    for a, b in zip(after_x0, before_x0):
        assert torch.equal(a, b)


@torch.no_grad()
def _tiny_img2img_loop(unet_w, unet_cfg, oracle, sched, pe, ne, images, n, strength, gs, generator):
    """tests/vae_encoder_oracle.img2img_loop with the tiny oracle as the encoder: its output is the initial latents as it is,
    nothing is drawn for a posterior, the forward noise is the generator's first draw."""
    from oracle.unet import unet_forward
    from tests.vae_encoder_oracle import add_noise_coefs
    t_start = max(n - min(int(n * strength), n), 0)
    ctx = torch.cat([ne, pe])
    sched.set_timesteps(n)
    timesteps = [int(t) for t in sched.timesteps][t_start:]
    init = oracle.encode01(images)
    noise = torch.randn(init.shape, generator=generator)
    alpha, sigma = add_noise_coefs(sched, t_start)
    start = alpha * init + sigma * noise
    latents = start.clone()
    for t in timesteps:
        u, c = unet_forward(unet_w, unet_cfg, torch.cat([latents] * 2), torch.tensor(t), ctx).chunk(2)
        latents = sched.step(u + gs * (c - u), t, latents, return_dict=False)[0]
    return latents, start, len(timesteps)


def test_img2img_with_the_tiny_encoder(env):
    from oracle.schedulers import DDIMOracle
    cfg, sd, model = env
    _, pe, ne = synth_inputs(cfg, 1, seed=81)
    img = _image(1, 128, 128, seed=82)
    model.load_tiny_vae("madebyollin/taesd", use_for="all")
    try:
        # the stand-in of the hub name is seeded by the name: the oracle gets the weights the model uses
        from tests import taesd_oracle as O
        oracle = O.build(model._tiny_state_dict())
        out, _, x0s = model(prompt_embeds=pe, negative_prompt_embeds=ne, image=img, strength=0.5, num_inference_steps=4,
                            guidance_scale=7.5, generator=torch.Generator().manual_seed(83), output_type="latent",
                            sample_mode="sample")
        ref, ref_start, steps = _tiny_img2img_loop(sd, oracle_cfg(cfg), oracle, DDIMOracle(), pe, ne, img, 4, 0.5, 7.5,
                                                   torch.Generator().manual_seed(83))
    finally:
        model.unload_tiny_vae()
    assert steps == 2 == model.num_timesteps == len(x0s)
    es, cs = rel_l2(model.img2img_start_latents, ref_start), cosine(model.img2img_start_latents, ref_start)
    e, c = rel_l2(out.images, ref), cosine(out.images, ref)
    print(f"img2img with the tiny encoder: start rel-L2 {es:.3e} cos {cs:.6f}; final rel-L2 {e:.3e} cos {c:.5f}")
    assert es < ENC_TOL and cs > ENC_COS
    assert e < FREE_TOL and c > FREE_COS
