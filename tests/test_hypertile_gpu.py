"""HyperTile on the GPU: the gather / scatter kernel of csrc/hypertile.hip against torch bit for bit, the attention op at the
shapes a tiled block hands it, the UNet forward against the tiled oracle (tests/hypertile_oracle.py), off-is-off, the DeepCache
skip plan, and the combinations with T-GATE, an IP-Adapter, a ControlNet, FreeU and the pipeline.

Tolerances.  Gather and scatter are copies: bit-exact.  The attention op: ATTN_TOL of tests/test_tome_gpu.py (P is rounded to
bf16 before PV) plus the per-element bound of tests/bounds.py.  The UNet: UNET_TOL of tests/test_unet_gpu.py against the tiled
oracle -- and, so that this means the tiling happened, more than FLOOR = 5 x UNET_TOL away from the library's own untiled result
(tests/test_hypertile_cpu.py holds the oracle's own tiled-against-plain distance to the same floor at the same inputs)."""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from sonicdiffusionbayeslab_amd import _lib
from tests import hypertile_oracle as ho
from tests.bounds import attention_elementwise, check_guards, forget_guards, guarded, guarded_input
from tests.util import cosine, oracle_cfg, rel_l2, synth_inputs

UNET_TOL = 2e-2                     # tests/test_unet_gpu.py
FREE_TOL = 6e-2                     # tests/test_pipeline_gpu.py
ATTN_TOL = 1e-2                     # tests/test_tome_gpu.py (tests/test_ops_gpu.py::test_attention)
_KEEP = []


def stream():
    return torch.cuda.current_stream().cuda_stream


def P(t):
    _KEEP.append(t)
    return t.data_ptr()


@pytest.fixture(autouse=True)
def _drop_keep():
    yield
    torch.cuda.synchronize()
    _KEEP.clear()
    forget_guards()


@pytest.fixture(scope="module")
def sdlib():
    return _lib.load()


def bits(t):
    return t.contiguous().view(torch.int16).cpu()


def rows_bf16(B, rh, rw, C, seed):
    """[B, rh * rw, C] bf16 with every kind of bit pattern a copy must keep: normal values, zeros of both signs, an Inf, a NaN."""
    x = torch.randn(B, rh * rw, C, generator=torch.Generator().manual_seed(seed)).to(torch.bfloat16)
    x[0, 0, :4] = torch.tensor([0.0, -0.0, float("inf"), float("nan")], dtype=torch.bfloat16)
    return x


# ------------------------------------------------------------------------------------------------------ gather / scatter
#          B  rh   rw   C     nh nw  pitch
COPY = {"2x3-of-16x24-c320": (2, 16, 24, 320, 2, 3, 320),          # level 0 of a 128x192 px image, T = 8
        "2x2-of-8x8-c1280": (3, 8, 8, 1280, 2, 2, 1280),           # the widest row: three 64-vector pieces (160 vectors)
        "3x5-of-6x10-c64": (1, 6, 10, 64, 3, 5, 64),               # odd tile counts, 2x2-token tiles, 8 vectors per row
        "pitch-wider-than-the-row": (2, 16, 24, 320, 2, 3, 344),   # the raster side inside a wider buffer
        "4x4-of-128x128-c320": (1, 128, 128, 320, 4, 4, 320),      # 1024 px: 16384 rows, more than one pass of the capped grid
        "one-tile": (2, 6, 10, 64, 1, 1, 64)}                      # the identity map


@pytest.mark.parametrize("case", COPY)
def test_gather_and_scatter_are_bit_exact_with_guard_bands(sdlib, case):
    B, rh, rw, C, nh, nw, pitch = COPY[case]
    N = rh * rw
    x = rows_bf16(B, rh, rw, C, seed=N + C)
    g = ho.gather_index(rh, rw, nh, nw)
    want = x[:, g]                                                  # tile order, from the index map of the definition
    assert torch.equal(bits(want), bits(ho.to_tiles(x, rh, rw, nh, nw).reshape(B, N, C)))
    ld = None if pitch == C else pitch
    xin = guarded_input(x.reshape(B * N, C), torch.bfloat16, ld=ld)
    tiles = guarded((B * N, C), torch.bfloat16)
    _lib.check(sdlib.sd_op_hypertile_gather(stream(), P(xin), pitch, P(tiles), B, rh, rw, C, nh, nw))
    torch.cuda.synchronize()
    assert torch.equal(bits(tiles), bits(want.reshape(B * N, C))), "gather"
    # scatter of the gather's own output is the identity; its output sits at the pitch too
    back = guarded((B * N, C), torch.bfloat16, ld=ld)
    _lib.check(sdlib.sd_op_hypertile_scatter(stream(), P(tiles), P(back), pitch, B, rh, rw, C, nh, nw))
    torch.cuda.synchronize()
    assert torch.equal(bits(back), bits(x.reshape(B * N, C))), "scatter of gather"
    # scatter on its own, from other rows
    y = rows_bf16(B, rh, rw, C, seed=N + C + 1)
    out = guarded((B * N, C), torch.bfloat16, ld=ld)
    _lib.check(sdlib.sd_op_hypertile_scatter(stream(), P(guarded_input(y.reshape(B * N, C), torch.bfloat16)), P(out), pitch, B, rh, rw, C, nh, nw))
    torch.cuda.synchronize()
    assert torch.equal(bits(out), bits(y[:, ho.scatter_index(rh, rw, nh, nw)].reshape(B * N, C))), "scatter"
    check_guards()


def test_row_offsets_past_2_to_the_31_elements(sdlib):
    """32768 rows at a pitch of 65552 elements: the last row starts at element 2 147 876 464 > 2^31 (byte 4.29e9 > 2^32), so a
    32-bit row offset -- in elements or in bytes -- lands elsewhere.  The raster buffer is never filled or read whole: the rows'
    C = 64 channels and an 8-element sentinel behind each are written through a strided view."""
    B, rh, rw, C, nh, nw, pitch = 2, 128, 128, 64, 4, 4, 65552
    rows = B * rh * rw
    assert (rows - 1) * pitch > 2 ** 31 and sdlib.sd_hypertile_check(B, rh, rw, C, nh, nw, pitch) == 0
    x = torch.randn(B, rh * rw, C, generator=torch.Generator().manual_seed(7)).to(torch.bfloat16)
    buf = torch.empty(rows * pitch, dtype=torch.bfloat16, device="cuda")
    view = buf.view(rows, pitch)
    view[:, :C] = x.reshape(rows, C).cuda()
    tiles = guarded((rows, C), torch.bfloat16)
    _lib.check(sdlib.sd_op_hypertile_gather(stream(), P(buf), pitch, P(tiles), B, rh, rw, C, nh, nw))
    torch.cuda.synchronize()
    assert torch.equal(bits(tiles), bits(x[:, ho.gather_index(rh, rw, nh, nw)].reshape(rows, C)))
    view[:, :C + 8] = -7.0                                          # the rows and a sentinel behind each
    _lib.check(sdlib.sd_op_hypertile_scatter(stream(), P(tiles), P(buf), pitch, B, rh, rw, C, nh, nw))
    torch.cuda.synchronize()
    assert torch.equal(bits(view[:, :C]), bits(x.reshape(rows, C)))
    assert bool((view[:, C:C + 8] == -7.0).all())
    check_guards()


def test_the_ops_refuse_what_sd_hypertile_check_refuses_and_write_nothing(sdlib):
    B, rh, rw, C, nh, nw = 2, 16, 24, 320, 2, 3
    N = rh * rw
    x = rows_bf16(B, rh, rw, C, seed=1)
    bad = [dict(B=0), dict(rh=0, nh=1), dict(rw=257, nw=1), dict(nh=3), dict(nw=5), dict(nh=0), dict(C=324), dict(C=0), dict(pitch=312),
           dict(pitch=324)]
    for kw in bad:
        a = dict(B=B, rh=rh, rw=rw, C=C, nh=nh, nw=nw, pitch=C)
        a.update(kw)
        assert sdlib.sd_hypertile_check(a["B"], a["rh"], a["rw"], a["C"], a["nh"], a["nw"], a["pitch"]) == -1, kw
        xin = guarded_input(x.reshape(B * N, C), torch.bfloat16)
        out = guarded((B * N, C), torch.bfloat16, fill=3.0)
        shape = (a["B"], a["rh"], a["rw"], a["C"], a["nh"], a["nw"])
        assert sdlib.sd_op_hypertile_gather(stream(), P(xin), a["pitch"], P(out), *shape) == -1, kw
        assert sdlib.sd_last_error().decode().startswith("hypertile_gather:"), (kw, sdlib.sd_last_error())
        assert sdlib.sd_op_hypertile_scatter(stream(), P(xin), P(out), a["pitch"], *shape) == -1, kw
        assert sdlib.sd_last_error().decode().startswith("hypertile_scatter:"), (kw, sdlib.sd_last_error())
        torch.cuda.synchronize()
        assert bool((out == 3.0).all()) and torch.equal(bits(xin), bits(x.reshape(B * N, C))), kw
    # null and unaligned pointers
    xin = guarded_input(x.reshape(B * N, C), torch.bfloat16)
    out = guarded((B * N, C), torch.bfloat16, fill=3.0)
    assert sdlib.sd_op_hypertile_gather(stream(), None, C, P(out), B, rh, rw, C, nh, nw) == -1
    assert sdlib.sd_op_hypertile_gather(stream(), P(xin) + 2, C, P(out), B, rh, rw, C, nh, nw) == -1
    assert "pointer" in sdlib.sd_last_error().decode()
    assert sdlib.sd_op_hypertile_scatter(stream(), P(xin), None, C, B, rh, rw, C, nh, nw) == -1
    assert sdlib.sd_op_hypertile_scatter(stream(), P(xin), P(out) + 8, C, B, rh, rw, C, nh, nw) == -1
    torch.cuda.synchronize()
    assert bool((out == 3.0).all())
    check_guards()


# ----------------------------------------------------------------------------------------------- attention at tiled shapes
# (d, heads, B = UNet batch x tiles, keys per tile).  d = 40: level 0 of SD 1.x; d = 80: its level 1; d = 64: SD 2.x with 5 heads
# on level 0 and 10 on level 1.  B = 36 = 4 x 9 and 144 = 16 x 9 / 9 x 16; 64 keys = 8x8-token tiles (the test UNets), 256 =
# 16x16, 1024 = 32x32 (tile_size 256).  q, k and v interleaved in one buffer with row stride 3 C, as the plan passes its q|k|v
# GEMM's output; the d = 40 cases with >= 256 keys ALSO through the head-major K / V entry, the form the plan then uses.
TILED_ATTN = [(40, 8, 36, 1024), (40, 8, 144, 256), (40, 8, 144, 64), (80, 8, 36, 256), (80, 8, 144, 64), (80, 8, 36, 1024),
              (64, 5, 36, 256), (64, 10, 144, 64), (64, 5, 36, 1024)]


@pytest.mark.parametrize("D,heads,B,Nk", TILED_ATTN)
def test_attention_at_tiled_shapes(sdlib, D, heads, B, Nk):
    """The result is compared on four tiles -- the first, the last and the two at B // 3 and 2 B // 3 -- against SDPA (rel-L2)
    and per element (tests/bounds.py); on all tiles it must be finite, and the guard bands round input and output hold.  The
    other tiles are skipped to keep the CPU time down."""
    C = heads * D
    g = torch.Generator().manual_seed(Nk * 8 + D + heads + B)
    q, k, v = (torch.randn(B, Nk, C, generator=g).to(torch.bfloat16).float() for _ in range(3))
    sel = [0, B // 3, 2 * B // 3, B - 1]
    qs, ks, vs = q[sel], k[sel], v[sel]
    qh, kh, vh = (t.view(len(sel), Nk, heads, D).transpose(1, 2) for t in (qs, ks, vs))
    ref = F.scaled_dot_product_attention(qh, kh, vh).transpose(1, 2).reshape(len(sel), Nk, C)
    qkv = guarded_input(torch.cat([q, k, v], dim=-1).reshape(B * Nk, 3 * C), torch.bfloat16)
    out = guarded((B, Nk, C), torch.bfloat16)
    base = P(qkv)
    _lib.check(sdlib.sd_op_attention(stream(), base, 3 * C, base + 2 * C, 3 * C, base + 4 * C, 3 * C, P(out), C, B, heads, Nk, Nk, D,
                                     1.0 / math.sqrt(D)))
    torch.cuda.synchronize()
    got = out.float().cpu()
    err = rel_l2(got[sel], ref)
    print(f"[hypertile attention] d={D} heads={heads} B={B} Nk={Nk}: rel-L2 on tiles {sel} {err:.3e}")
    assert torch.isfinite(got).all() and err < ATTN_TOL
    attention_elementwise(out[sel], qs, ks, vs, heads, D, f"attention tiled d{D} h{heads} B={B} Nk={Nk} tiles {sel}")
    if D == 40 and Nk >= 256:
        khm, vhm = (guarded_input(t.view(B, Nk, heads, D).permute(0, 2, 1, 3).contiguous(), torch.bfloat16) for t in (k, v))
        qd = guarded_input(q.reshape(B * Nk, C), torch.bfloat16)
        out2 = guarded((B, Nk, C), torch.bfloat16)
        _lib.check(sdlib.sd_op_attention_headmajor(stream(), P(qd), C, P(khm), P(vhm), P(out2), C, B, heads, Nk, Nk, D, 1.0 / math.sqrt(D)))
        torch.cuda.synchronize()
        got2 = out2.float().cpu()
        err2 = rel_l2(got2[sel], ref)
        print(f"[hypertile attention] ... head-major K / V: rel-L2 {err2:.3e}")
        assert torch.isfinite(got2).all() and err2 < ATTN_TOL
        attention_elementwise(out2[sel], qs, ks, vs, heads, D, f"attention tiled head-major B={B} Nk={Nk} tiles {sel}")
    check_guards()


# ------------------------------------------------------------------------------------------------------------- the UNet
_NETS = {}


def net_of(name):
    from sonicdiffusionbayeslab_amd.unet import HipUNet2DConditionModel
    if name not in _NETS:
        cfg, sd, ocfg, heads = ho.env(name)
        _NETS[name] = HipUNet2DConditionModel(cfg, sd)
    return _NETS[name]


def gpu_forward(net, lat, ctx, ub, t, h, w, setting):
    """eps of the library with HyperTile at ``setting`` = (tile_tokens, max_depth) or None = off; leaves the handle off."""
    net.set_deepcache(-1)
    net.set_hypertile(*(setting or (0, 0)))
    try:
        net.set_context(ctx.cuda(), h, w)
        eps = net.forward_latents(lat.cuda(), ub, t).clone()
        torch.cuda.synchronize()
        return eps.cpu()
    finally:
        net.set_hypertile(0)


def forward_tiled_and_check(case):
    name, h, w, lb, ub, seed, t, T, md, n = case
    cfg = ho.env(name)[0]
    net = net_of(name)
    lat, ctx, _ = ho.unet_inputs(cfg, h, w, lb, ub, seed)
    ref = ho.reference(case)
    net.set_hypertile(T, md)
    try:
        blocks = net.hypertile_blocks(h, w)
    finally:
        net.set_hypertile(0)
    assert [(b["rh"], b["rw"], b["nh"], b["nw"]) for b in blocks] == ref["used"] and len(blocks) == n     # the oracle's call order
    assert net.hypertile_blocks(h, w) == []
    eps = gpu_forward(net, lat, ctx, ub, t, h, w, (T, md))
    own_plain = gpu_forward(net, lat, ctx, ub, t, h, w, None)
    err, err_plain = rel_l2(eps, ref["tiled"]), rel_l2(own_plain, ref["plain"])
    moved, own = rel_l2(eps, own_plain), rel_l2(ref["tiled"], ref["plain"])
    print(f"[hypertile unet] {name} {h}x{w} batch {lb}/{ub} T {T} max_depth {md}: rel-L2 vs the tiled oracle {err:.3e} cos "
          f"{cosine(eps, ref['tiled']):.5f}; untiled vs the plain oracle {err_plain:.3e}; tiled vs the library's own untiled {moved:.3f} "
          f"(the oracle's own {own:.3f}, floor {ho.FLOOR:.2f})")
    assert own > ho.FLOOR
    assert torch.isfinite(eps).all() and err < UNET_TOL
    assert err_plain < UNET_TOL
    assert moved > ho.FLOOR
    return blocks


def _ids(cases):
    return [f"{c[1]}x{c[2]}-b{c[3]}_{c[4]}-T{c[7]}-d{c[8]}" for c in cases]


SD15 = [c for c in ho.UNET_CASES if c[0] == "sd15"]
TWO_LEVEL = [c for c in ho.UNET_CASES if c[0] == "two_level"]


@pytest.mark.parametrize("case", SD15, ids=_ids(SD15))
def test_unet_forward_matches_the_tiled_oracle(case):
    """16x16 and 16x24 latents: level 0 in 2x2 / 2x3 tiles of 64 tokens, under a CFG pair (the first block gathers once per
    latent and the replicate copies the tile-ordered tensors).  32x32 at max_depth 2: 4x4 tiles on level 0 (fused prompt
    cross-attention, 1024 rows per sample), 2x2 on level 1 (640 channels), level 2 in one tile and so not tiled."""
    forward_tiled_and_check(case)


def head_major(lib, C, heads, UB, tiles, Na):
    """csrc/plan.hip, Builder::transformer_block: the q|k|v GEMM of a block stores K / V head-major, and attn_pipe40_kernel reads
    them, when all of this holds -- Na = the keys of one tile, M = UB x tiles x Na rows."""
    M = UB * tiles * Na
    return (C // heads == 40 and C % 160 == 0 and Na % 128 == 0 and Na >= 256 and lib.sd_op_gemm_tile_rows(M, 3 * C, 0) == 128
            and lib.sd_op_gemm_splitk(M, 3 * C, C, 0) == 1)


@pytest.mark.parametrize("case", TWO_LEVEL, ids=_ids(TWO_LEVEL))
def test_unet_forward_tiled_on_and_off_the_head_major_path(sdlib, case):
    """32x32 latents on the 320 / 640 UNet, 16 samples of 8 latents.  T = 16: level 0 runs 2x2 tiles of 256 keys and all five of
    its blocks -- the first on the 8 samples of the CFG prefix, 8192 rows, the others on 16 -- store K / V head-major and run
    attn_pipe40_kernel on 256-key tiles (untiled, the same blocks run it on 1024 keys).  T = 8, max_depth 1: 64-key tiles on both
    levels, below the kernel's 256-key minimum -- the SAME blocks then take the token-major path, the other side of the
    predicate; level 1 and the mid block (640 channels, d = 80) never take it."""
    name, h, w, lb, ub, seed, t, T, md, n = case
    cfg = ho.env(name)[0]
    C, heads = cfg.block_out_channels[0], cfg.num_heads
    nh, nw, th, tw = ho.tiling(h, w, T)
    want = [head_major(sdlib, C, heads, u, nh * nw, th * tw) for u in (lb, ub)]
    assert want == ([True, True] if T == 16 else [False, False]) and th * tw == {16: 256, 8: 64}[T]
    assert head_major(sdlib, C, heads, ub, 1, h * w)                                  # untiled: head-major on 1024 keys
    assert not head_major(sdlib, cfg.block_out_channels[1], heads, ub, 4, 64)
    blocks = forward_tiled_and_check(case)
    assert [(b["rh"], b["rw"]) for b in blocks].count((32, 32)) == 5
    prof_net = net_of(name)
    lat, ctx, _ = ho.unet_inputs(cfg, h, w, lb, ub, seed)
    prof_net.set_hypertile(T, md)
    try:
        prof_net.set_context(ctx.cuda(), h, w)
        prof = prof_net.forward_profiled(lat.cuda(), ub, t)
    finally:
        prof_net.set_hypertile(0)
    prof_net.set_context(ctx.cuda(), h, w)
    plain = prof_net.forward_profiled(lat.cuda(), ub, t)
    assert prof["hypertile_gather"]["launches"] == prof["hypertile_scatter"]["launches"] == n and prof["hypertile_gather"]["bytes"] > 0
    assert "hypertile_gather" not in plain and "hypertile_scatter" not in plain
    # every fold of the plain plan is kept: the same launch count of every other kind
    for kind in ("gemm", "attention", "layernorm", "groupnorm", "xattn_fused", "replicate", "conv3x3"):
        assert prof.get(kind, {"launches": 0})["launches"] == plain.get(kind, {"launches": 0})["launches"], kind


def test_sd2_shaped_unet_forward_tiled():
    """The SD 2.x-shaped UNet (5 / 10 / 20 / 20 heads of 64) at 16x16, T = 8."""
    forward_tiled_and_check(ho.SD2_CASE)


def test_off_is_off_and_the_deepcache_skip_plan_tiles():
    from sonicdiffusionbayeslab_amd.unet import CACHE_FULL_AND_STORE, CACHE_SKIP, HipUNet2DConditionModel
    cfg, sd, _, _ = ho.env("sd15")
    lat, pe, ne = synth_inputs(cfg, 1)
    ctx = torch.cat([ne, pe])
    fresh = HipUNet2DConditionModel(cfg, sd)                # a handle that never sees the setting
    fresh.set_deepcache(-1)
    fresh.set_context(ctx.cuda())
    never = fresh.forward_latents(lat.cuda(), 2, 501.0).clone().cpu()
    never_bytes = [fresh._workspace_bytes(2, br, 16, 16) for br in (-1, 0)]
    net = net_of("sd15")
    a = gpu_forward(net, lat, ctx, 2, 501.0, 16, 16, None)
    on = gpu_forward(net, lat, ctx, 2, 501.0, 16, 16, (8, 0))
    on2 = gpu_forward(net, lat, ctx, 2, 501.0, 16, 16, (8, 0))
    net.set_hypertile(8, 0)
    on_bytes = net._workspace_bytes(2, -1, 16, 16)
    net.set_hypertile(0)
    b = gpu_forward(net, lat, ctx, 2, 501.0, 16, 16, None)
    assert torch.equal(a, never) and torch.equal(b, never) and torch.equal(on, on2) and not torch.equal(on, never)
    assert [net._workspace_bytes(2, br, 16, 16) for br in (-1, 0)] == never_bytes and on_bytes > 0
    # a setting that tiles nothing at this size (one tile per level) builds plans of its own that compute the same
    assert torch.equal(gpu_forward(net, lat, ctx, 2, 501.0, 16, 16, (16, 3)), never)
    # DeepCache branch 0: the skip step runs up_blocks.3.attentions.2 alone of the five tiled blocks.  block_info reports the
    # FULL plan (which blocks tile depends on the size and the setting alone: the same five under any branch); that the skip
    # step's one block ran tiled is read from the skip step's own launches, one gather and one scatter
    net.set_hypertile(8, 0)
    net.set_deepcache(0)
    try:
        assert net.hypertile_blocks(16, 16) == [dict(rh=16, rw=16, nh=2, nw=2)] * 5
        net.set_context(ctx.cuda())
        full = net.forward_latents(lat.cuda(), 2, 501.0, cache_mode=CACHE_FULL_AND_STORE).clone().cpu()
        skip = net.forward_latents(lat.cuda(), 2, 481.0, cache_mode=CACHE_SKIP).clone().cpu()
        net.forward_profiled(lat.cuda(), 2, 501.0, cache_mode=CACHE_FULL_AND_STORE)
        prof = net.forward_profiled(lat.cuda(), 2, 481.0, cache_mode=CACHE_SKIP)
    finally:
        net.set_hypertile(0)
    net.set_context(ctx.cuda())
    full0 = net.forward_latents(lat.cuda(), 2, 501.0, cache_mode=CACHE_FULL_AND_STORE).clone().cpu()
    skip0 = net.forward_latents(lat.cuda(), 2, 481.0, cache_mode=CACHE_SKIP).clone().cpu()
    net.set_deepcache(-1)
    assert torch.isfinite(full).all() and torch.isfinite(skip).all()
    assert prof["hypertile_gather"]["launches"] == prof["hypertile_scatter"]["launches"] == 1
    print(f"[hypertile deepcache] full step tiled vs untiled {rel_l2(full, full0):.3f}; skip step {rel_l2(skip, skip0):.3f}")
    assert rel_l2(full, full0) > ho.FLOOR and rel_l2(skip, skip0) > UNET_TOL


def test_refusals_on_the_handle():
    net = net_of("sd15")
    with pytest.raises(ValueError, match="tile_tokens"):
        net.set_hypertile(4)
    with pytest.raises(ValueError, match="max_depth"):
        net.set_hypertile(8, 5)
    net.set_tome(0.5, 1)
    try:
        with pytest.raises(NotImplementedError, match="Token Merging"):
            net.set_hypertile(8)
    finally:
        net.set_tome(0.0)
    net.set_hypertile(8)
    try:
        with pytest.raises(NotImplementedError, match="HyperTile"):
            net.set_tome(0.5, 1)
        # the library's own refusal, below the wrapper
        assert net._lib.sd_unet_set_tome(net._handle, 0.5, 1) == -1 and "HyperTile" in net._lib.sd_last_error().decode()
        assert net._lib.sd_unet_set_hypertile(net._handle, 4, 0) == -1 and net._lib.sd_unet_set_hypertile(net._handle, 8, 4) == -1
    finally:
        net.set_hypertile(0)
    assert net.hypertile_blocks(16, 16) == []


# --------------------------------------------------------------------------------------------------------- combinations
def test_with_tgate_the_capturing_and_gated_forwards_match_the_composed_oracle():
    """T-GATE composed with the tiled block at 16x16, CFG pair of 2 latents: the capture forward (batch 4) writes the cache in
    tile order, the gated forward (batch 2, other latents, another timestep) adds it in the same order -- a gated forward whose
    rows did not line up would be far from the oracle, whose cache is in raster order throughout."""
    from tests import tgate_oracle as tg
    case = tg.CASES[0]
    _, name, h, w, lb, cfg_on, _, t0, t1 = case
    cfg, sd, ocfg, heads = tg.env(name)
    net = net_of(name)
    lat0, lat1, ctx = tg.inputs(case)
    ub = ctx.shape[0]
    st = tg.TGateState(2)
    with ho.patched(ho.TileRun((h, w), 8, 0)):
        ref_cap = tg.unet_forward(sd, ocfg, torch.cat([lat0] * 2), t0, ctx, st, "capture")
        ref_gated = tg.unet_forward(sd, ocfg, lat1, t1, ctx[-lb:], st, "reuse")
    untiled = tg.reference(case)
    net.set_deepcache(-1)

    def run(setting):
        net.set_hypertile(*(setting or (0, 0)))
        try:
            net.set_tgate(net.TGATE_CAPTURE, lb, h, w)
            net.set_context(ctx.cuda(), h, w)
            c = net.forward_latents(lat0.cuda(), ub, t0).clone().cpu()
            net.set_tgate(net.TGATE_REUSE, lb, h, w)
            return c, net.forward_latents(lat1.cuda(), lb, t1).clone().cpu()
        finally:
            net.set_tgate(net.TGATE_OFF)
            net.set_hypertile(0)
    # off first, then on, on ONE handle at one batch and size -- what methods_registry["hypertile"] does with model.tgate_step:
    # the workspace of the gated plans must not outlive the setting it was sized for (set_hypertile drops it)
    _, gated_off = run(None)
    assert net._tgate_ws.tensor is not None          # (kept while the setting does not change ...)
    cap, gated = run((8, 0))
    assert net._tgate_ws.tensor is None              # (... dropped when it does: here by the switch back to off)
    assert rel_l2(gated_off, untiled["gated"]) < UNET_TOL
    e_cap, e_gated = rel_l2(cap, ref_cap), rel_l2(gated, ref_gated)
    print(f"[hypertile + tgate] capture {e_cap:.3e}, gated {e_gated:.3e}; the oracle's tiled vs untiled gated {rel_l2(ref_gated, untiled['gated']):.3f}")
    assert rel_l2(ref_gated, untiled["gated"]) > ho.FLOOR
    assert torch.isfinite(gated).all() and e_cap < UNET_TOL and e_gated < UNET_TOL


def test_with_an_ip_adapter():
    from oracle.unet import unet_forward
    from sonicdiffusionbayeslab_amd.unet import HipUNet2DConditionModel
    from sonicdiffusionbayeslab_amd.weights import UNetConfig, make_synthetic_ip_adapter_state_dict, make_synthetic_state_dict
    from tests.ip_adapter_oracle import cfg_image_embeds, ip_adapter_oracle
    from tests.tome_oracle import tome_test_weights
    E = 64
    cfg = UNetConfig(sample_size=16, ip_adapter_embed_dim=E)
    sd = tome_test_weights(make_synthetic_state_dict(cfg, seed=1234))
    w = {**sd, **make_synthetic_ip_adapter_state_dict(cfg, seed=1234)}
    net = HipUNet2DConditionModel(cfg, w)
    lat, pe, ne = synth_inputs(cfg, 2)
    emb = cfg_image_embeds(torch.randn(2, E, generator=torch.Generator().manual_seed(3)), True)
    ctx, lat_in, t = torch.cat([ne, pe]), torch.cat([lat, lat]), 981.0
    with torch.no_grad(), ip_adapter_oracle(w, emb, 1.0):
        plain = unet_forward(w, oracle_cfg(cfg), lat_in, t, ctx)
        ref = ho.unet_forward(w, oracle_cfg(cfg), lat_in, t, ctx, ho.TileRun((16, 16), 8, 0))
    net.set_deepcache(-1)
    net.set_hypertile(8, 0)
    try:
        net.set_context(ctx.cuda())
        net.set_ip_adapter(emb, 1.0)
        eps = net.forward_latents(lat.cuda(), 4, t).clone().cpu()
    finally:
        net.clear_ip_adapter()
        net.set_hypertile(0)
    err = rel_l2(eps, ref)
    print(f"[hypertile + ip-adapter] rel-L2 {err:.3e}; the oracle's tiled vs untiled {rel_l2(ref, plain):.3f}")
    assert rel_l2(ref, plain) > ho.FLOOR and torch.isfinite(eps).all() and err < UNET_TOL


def test_with_a_controlnet_whose_own_handle_never_tiles():
    from sonicdiffusionbayeslab_amd.controlnet import HipControlNetModel
    from sonicdiffusionbayeslab_amd.weights import controlnet_config_for, make_synthetic_controlnet_state_dict
    from tests.controlnet_oracle import controlled_unet_forward
    cfg, sd, ocfg, _ = ho.env("sd15")
    cn = controlnet_config_for(cfg)
    cw = make_synthetic_controlnet_state_dict(cn, seed=1234)
    cnet, net = HipControlNetModel(cn, cw), net_of("sd15")
    h, w, t = 16, 24, 981.0
    g = torch.Generator().manual_seed(30)
    lat, ctx = torch.randn(1, 4, h, w, generator=g), torch.randn(2, 77, 768, generator=g)
    cond = torch.rand(1, 3, 8 * h, 8 * w, generator=torch.Generator().manual_seed(31))
    lat_in = torch.cat([lat, lat])
    run = ho.TileRun((h, w), 8, 0)
    with torch.no_grad():
        ref = controlled_unet_forward(sd, cw, ocfg, lat_in, t, ctx, cond, 1.0, unet_ctx=lambda: ho.patched(run))
        plain = controlled_unet_forward(sd, cw, ocfg, lat_in, t, ctx, cond, 1.0)
    assert len(run.used) == 5                               # the UNet's five level-0 blocks; none of the ControlNet's
    cnet.set_context(ctx.cuda(), h, w)
    cnet.set_cond(cond)
    buf = cnet.forward_residuals(lat.cuda(), 2, t)
    net.set_deepcache(-1)
    net.set_hypertile(8, 0)
    try:
        net.set_context(ctx.cuda(), h, w)
        net.set_control_residuals(buf, 1.0, 2, h, w)
        eps = net.forward_latents(lat.cuda(), 2, t).clone().cpu()
    finally:
        net.clear_control_residuals()
        net.set_hypertile(0)
    err = rel_l2(eps, ref)
    print(f"[hypertile + controlnet] rel-L2 {err:.3e}; the oracle's tiled vs untiled {rel_l2(ref, plain):.3f}")
    assert rel_l2(ref, plain) > ho.FLOOR and torch.isfinite(eps).all() and err < UNET_TOL
    assert cnet._lib.sd_unet_set_hypertile(cnet._handle, 8, 0) == -1 and "not a UNet handle" in cnet._lib.sd_last_error().decode()


def test_with_freeu():
    from tests import freeu_oracle as fo
    cfg, sd, ocfg, _ = ho.env("sd15")
    net = net_of("sd15")
    h, w, lb, ub, t = 16, 16, 2, 4, 981.0
    lat, ctx, sample = ho.unet_inputs(cfg, h, w, lb, ub)
    with ho.patched(ho.TileRun((h, w), 8, 0)):
        ref = fo.unet_forward(sd, ocfg, sample, t, ctx, fo.GIVEN)
    tiled_only = ho.reference(ho.UNET_CASES[0])["tiled"]
    net.set_deepcache(-1)
    net.set_hypertile(8, 0)
    net.set_freeu(*fo.GIVEN)
    try:
        net.set_context(ctx.cuda(), h, w)
        eps = net.forward_latents(lat.cuda(), ub, t).clone().cpu()
    finally:
        net.disable_freeu()
        net.set_hypertile(0)
    err = rel_l2(eps, ref)
    print(f"[hypertile + freeu] rel-L2 {err:.3e}; the oracle with vs without FreeU, both tiled {rel_l2(ref, tiled_only):.3f}")
    assert rel_l2(ref, tiled_only) > ho.FLOOR and torch.isfinite(eps).all() and err < UNET_TOL


def test_pipeline_of_three_steps_at_a_non_square_size():
    """DDIM, three steps at 256x320 px (32x40 latents) with tile_size 64 (T = 8: 4x5 tiles on level 0) against the oracle's loop
    with the tiled block; off after on is the model that never saw the setting, bit for bit; image-to-image and DeepCache run.
    (The pipeline's size rule -- multiples of 64 in [256, 1024] -- does not admit the 128x192 px of 16x24 latents: that size runs
    at the UNet level above, in test_unet_forward_matches_the_tiled_oracle and the ControlNet combination; 256x320 px is the
    smallest non-square size a pipeline call takes.)"""
    from oracle.pipeline import sample_loop
    from oracle.schedulers import DDIMOracle
    from sonicdiffusionbayeslab_amd.models import StableDiffusionModel
    from sonicdiffusionbayeslab_amd.registry import schedulers_registry
    cfg, sd, ocfg, _ = ho.env("sd15")
    model = StableDiffusionModel(unet_config=cfg, state_dict=dict(sd)).to("cuda:0")
    model.scheduler = schedulers_registry["ddim_scheduler"].from_config(model.scheduler.config)
    g = torch.Generator().manual_seed(29)
    lat = torch.randn((1, 4, 32, 40), generator=g)
    pe, ne = torch.randn((1, 77, 768), generator=g), torch.randn((1, 77, 768), generator=g)

    def call(**kw):
        args = dict(prompt_embeds=pe, negative_prompt_embeds=ne, num_inference_steps=3, guidance_scale=7.5, output_type="latent",
                    height=256, width=320)
        if "image" not in kw:
            args["latents"] = lat
        args.update(kw)
        return model(**args)[0].images.float().cpu()
    plain = call()
    assert model.enable_hypertile(tile_size=64) is model
    on = call()
    with torch.no_grad():
        with ho.patched(ho.TileRun((32, 40), 8, 0)):
            ref = sample_loop(sd, ocfg, DDIMOracle(), pe, ne, lat, 3, 7.5)[0]
        ref_plain = sample_loop(sd, ocfg, DDIMOracle(), pe, ne, lat, 3, 7.5)[0]
    err, moved, own = rel_l2(on, ref), rel_l2(on, plain), rel_l2(ref, ref_plain)
    print(f"[hypertile pipeline] 3-step DDIM at 32x40 latents: rel-L2 vs the tiled oracle loop {err:.3e}; tiled vs plain {moved:.3f} (the "
          f"oracle's own {own:.3f}); plain vs its oracle {rel_l2(plain, ref_plain):.3e}")
    assert torch.isfinite(on).all() and err < FREE_TOL and own > 2 * FREE_TOL and moved > FREE_TOL
    assert torch.equal(call(), on)
    from sonicdiffusionbayeslab_amd.deepcache import DeepCacheSDHelper
    helper = DeepCacheSDHelper(pipe=model)
    helper.set_params(cache_interval=2, cache_branch_id=0)
    helper.enable()
    try:
        dc = call(num_inference_steps=4)
    finally:
        helper.disable()
    assert torch.isfinite(dc).all()
    img = torch.rand(1, 3, 256, 320, generator=torch.Generator().manual_seed(8))
    i2i = call(num_inference_steps=4, image=img, strength=0.5, generator=torch.Generator().manual_seed(1))
    assert torch.isfinite(i2i).all() and i2i.shape == (1, 4, 32, 40)
    assert model.disable_hypertile() is model
    assert torch.equal(call(), plain)
