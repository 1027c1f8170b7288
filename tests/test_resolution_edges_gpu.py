"""The image sizes the height / width rule accepts beyond the ones test_resolution_gpu.py covers: latent sides 32..128 in
steps of 8, where UNet levels have odd sides (5x5, 5x7, 7x9), extreme aspect ratios (4x16 next to 32x128) and token
counts that are not multiples of 128 (25, 35, 63, 140, 252, 400, 560, 1008, 1600, 2240, 4032).  Every kernel is driven at
the exact shapes the plan builds for those sizes and compared with a plain fp32 / fp64 torch reference on bf16-rounded
inputs; then the whole UNet, the VAE decoder and one pipeline run against the CPU oracle (oracle/*.py) at those sizes.

Gates are those of the tests these mirror: OP_TOL (test_ops_gpu.py: one kernel, bf16 output rounding), 1e-2 for attention
(P is rounded to bf16 before PV), UNET_TOL for one UNet forward, FREE_TOL / FREE_COS for sampling loops, the fp8 gates of
test_fp8_gpu.py and the VAE gate of test_vae_gpu.py."""
import math
import os

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from sonicdiffusionbayeslab_amd import _lib
from tests.util import cosine, oracle_cfg, rel_l2
from tests.bounds import (ATOL_TINY, U32, NHWC, assert_e4m3_codes, assert_elementwise, assert_flip_budget,
                          attention_elementwise, check_guards, conv3x3_nhwc_ref, conv_gn_elementwise, device_operand,
                          forget_guards, fp8_conv_ref, fp8_gemm_ref_bound, geglu_ref_bound, gemm_bound, gn_restatements,
                          grouped_softmax_elementwise, guarded,
                          guarded_input, linear_bound, ln_fold_elementwise, ln_fold_ref_bound, norm_ref_bound, sample_rows,
                          softmax_rows_ref_bound, softmax_rows_elementwise, subpixel_ref, ulp_bf16,
                          xattn_elementwise, xattn_norm2_elementwise)

OP_TOL = 6e-3                     # test_ops_gpu.py / test_fp8_gpu.py: one kernel, bf16 output rounding
ATTN_TOL = 1e-2                   # test_ops_gpu.py::test_attention: P rounded to bf16 before PV
UNET_TOL = 2e-2                   # one UNet forward
FREE_TOL, FREE_COS = 6e-2, 0.998  # free-running loops

_KEEP = []


def stream():
    return torch.cuda.current_stream().cuda_stream


def P(t, dtype=None):
    """Upload (if needed) and return the device pointer, keeping the tensor alive until the test ends."""
    if t is None:
        return None
    t = device_operand(t, dtype)                  # guarded buffers as they are, anything else into a guarded copy
    _KEEP.append(t)
    return t.data_ptr()


@pytest.fixture(autouse=True)
def _drop_keep():
    yield
    torch.cuda.synchronize()
    _KEEP.clear()
    check_guards()              # every guard of every operand and output of the test (tests/bounds.py)


def r16(t):
    return t.to(torch.bfloat16).float()


def env_once(name, value, fn):
    """fn() with the environment switch `name` set (switches the library reads per call only)."""
    old = os.environ.get(name)
    os.environ[name] = value
    try:
        return fn()
    finally:
        if old is None:
            del os.environ[name]
        else:
            os.environ[name] = old


# ------------------------------------------------------------------------------------------ attention
def _dominant_key_case(g, B, heads, D, Nq, Nk, spikes):
    """test_ops_gpu.py's construction: queries share a component u, keys f * u at the given positions score ~18 f log2
    units above everything before them for every query (a real prompt's BOS key, an outlier channel)."""
    C = heads * D
    u = torch.ones(C)
    q = r16(torch.randn(B, Nq, C, generator=g) + 2.0 * u)
    k = r16(torch.randn(B, Nk, C, generator=g))
    v = r16(torch.randn(B, Nk, C, generator=g))
    for pos, f in spikes:
        k[:, pos] = r16(f * u * (math.sqrt(40.0 / D)) + 0.1 * k[:, pos])
    return q, k, v


# (B, Nq, Nk, D, spikes): the self-attentions of the odd UNet levels (d = 160 at the deepest two levels, d = 80 at level 1,
# d = 40 at level 0) and the 77-key cross-attention the "to_q GEMM + attention" form runs where neither fused form applies.
# Kernels (csrc/attention.hip::sd_launch_attention): d = 160 -> attn_kernel<160> (every key count; 25 / 35 / 63 < one
# 64-key tile); d = 80 with Nk % 64 != 0 -> attn_kernel<80> (not the pipelined one); d = 40 with Nk % 64 == 0 and
# >= 256 -> attn_pipe40_kernel (1600 / 2240 / 4032: multiples of 64, not of 128), 77 keys -> attn_dma_kernel<40>.
# spikes: dominant keys in the ragged LAST tile (position >= the last multiple of 64), as test_ops_gpu.py's spike cases.
ATTN_CASES = [
    (2, 25, 25, 160, ()), (2, 35, 35, 160, ()), (2, 63, 63, 160, ()), (2, 100, 100, 160, ()), (2, 140, 140, 160, ()),
    (2, 252, 252, 160, ()),
    (2, 25, 25, 160, ((3, 13.0), (23, 26.0))), (2, 140, 140, 160, ((9, 13.0), (130, 26.0), (139, 39.0))),
    (2, 400, 400, 80, ()), (2, 560, 560, 80, ()), (1, 1008, 1008, 80, ()),
    (2, 560, 560, 80, ((9, 13.0), (300, 26.0), (551, 39.0))),
    (1, 1600, 1600, 40, ()), (1, 2240, 2240, 40, ()), (1, 4032, 4032, 40, ()),
    (1, 2240, 2240, 40, ((13, 13.0), (1000, 26.0), (2239, 39.0))),
    (2, 25, 77, 160, ()), (2, 140, 77, 160, ()), (1, 2240, 77, 40, ()),
    (2, 140, 77, 160, ((5, 13.0), (70, 26.0), (76, 39.0))), (1, 2240, 77, 40, ((5, 13.0), (41, 26.0), (75, 39.0))),
]


@pytest.mark.parametrize("B,Nq,Nk,D,spikes", ATTN_CASES)
def test_attention_at_odd_level_token_counts(sdlib, B, Nq, Nk, D, spikes):
    heads = 8
    C = heads * D
    g = torch.Generator().manual_seed(Nq * 7 + Nk + D + len(spikes))
    if spikes:
        q, k, v = _dominant_key_case(g, B, heads, D, Nq, Nk, spikes)
    else:
        q, k, v = (r16(torch.randn(B, n, C, generator=g)) for n in (Nq, Nk, Nk))
    qh, kh, vh = (t.view(B, -1, heads, D).transpose(1, 2) for t in (q, k, v))
    if spikes:                                    # the construction really produces the jumps it claims
        s = (qh @ kh.transpose(-1, -2)) / math.sqrt(D) * 1.4426950408889634
        for pos, _ in spikes:
            assert (s[..., pos] - s[..., :pos].amax(-1)).min() > 150.0
    ref = F.scaled_dot_product_attention(qh, kh, vh).transpose(1, 2).reshape(B, Nq, C)
    kv = torch.cat([k, v], dim=-1).contiguous().to("cuda", torch.bfloat16)
    out = guarded((B, Nq, C), torch.bfloat16)
    kvp = P(kv)
    _lib.check(sdlib.sd_op_attention(stream(), P(q, torch.bfloat16), C, kvp, 2 * C, kvp + 2 * C, 2 * C, P(out), C, B,
                                     heads, Nq, Nk, D, 1.0 / math.sqrt(D)))
    torch.cuda.synchronize()
    err = rel_l2(out, ref)
    print(f"attention B={B} Nq={Nq} Nk={Nk} d={D} spikes={len(spikes)}: rel-L2 {err:.3e}")
    assert torch.isfinite(out.float()).all() and err < ATTN_TOL
    attention_elementwise(out, q, k, v, heads, D, f"attention odd tokens B={B} {Nq}x{Nk} d{D} spikes={len(spikes)}")


@pytest.mark.parametrize("B,N,Nk,D", [(2, 25, 25, 160), (2, 140, 140, 160), (2, 140, 77, 160), (2, 560, 560, 80), (2, 1008, 1008, 80),
                                     (1, 2240, 2240, 40), (1, 4032, 4032, 40), (1, 2240, 77, 40)])
def test_attention_moderate_key_spike_in_the_ragged_last_tile(sdlib, B, N, Nk, D):
    """A key three from the end scaled by 6 (test_ops_gpu.py::test_attention's spike): the running maximum jumps in the
    partial last tile while the probabilities stay spread over many keys, so a mis-masked or mis-rescaled tail shows in the
    output.  (The dominant-key cases above collapse every row onto one key: they prove no overflow, not the tail's sums.)"""
    heads = 8
    C = heads * D
    g = torch.Generator().manual_seed(N * 3 + Nk + D)
    q, k, v = (r16(torch.randn(B, n, C, generator=g)) for n in (N, Nk, Nk))
    k[:, Nk - 3] = r16(k[:, Nk - 3] * 6)
    qh, kh, vh = (t.view(B, -1, heads, D).transpose(1, 2) for t in (q, k, v))
    ref = F.scaled_dot_product_attention(qh, kh, vh).transpose(1, 2).reshape(B, N, C)
    kv = torch.cat([k, v], dim=-1).contiguous().to("cuda", torch.bfloat16)
    out = guarded((B, N, C), torch.bfloat16)
    kvp = P(kv)
    _lib.check(sdlib.sd_op_attention(stream(), P(q, torch.bfloat16), C, kvp, 2 * C, kvp + 2 * C, 2 * C, P(out), C, B,
                                     heads, N, Nk, D, 1.0 / math.sqrt(D)))
    torch.cuda.synchronize()
    err = rel_l2(out, ref)
    print(f"attention, key {Nk - 3} x6, B={B} Nq={N} Nk={Nk} d={D}: rel-L2 {err:.3e}")
    assert torch.isfinite(out.float()).all() and err < ATTN_TOL
    attention_elementwise(out, q, k, v, heads, D, f"attention ragged-tile spike B={B} {N}x{Nk} d{D}")


# ------------------------------------------------------------------------------------------ head-major q|k|v
# tokens per sample that are multiples of 128 but not powers of two: the head-major store of the GENERAL GEMM kernel
# (gemm_conv.hip; the lean kernel takes power-of-two token counts only).  Batches keep M >= 8192 rows: the plan (and
# check_headmajor) stores K / V head-major only on 128-row tiles (sd_gemm_tile_rows == 128, i.e. >= 384 tiles of 128 x 160).
@pytest.mark.parametrize("B,N", [(6, 1536), (3, 3840), (2, 6144)])
def test_qkv_projection_and_attention_head_major_at_non_power_of_two_tokens(sdlib, B, N):
    g = torch.Generator().manual_seed(N + B)
    C, H, D = 320, 8, 40
    M = B * N
    x = r16(torch.randn(M, C, generator=g))
    w = r16(torch.randn(3 * C, C, generator=g) / math.sqrt(C))
    qkv = r16(x @ w.t())
    q = guarded((M, C), torch.bfloat16)
    kv = guarded((2, B, H, N, D), torch.bfloat16)
    _lib.check(sdlib.sd_op_gemm_qkv_headmajor(stream(), P(x, torch.bfloat16), C, P(w, torch.bfloat16), P(q), P(kv), M, C, N, C))
    torch.cuda.synchronize()
    eq = rel_l2(q, qkv[:, :C])
    ekv = [rel_l2(kv[which], qkv[:, (1 + which) * C:(2 + which) * C].view(B, N, H, D).permute(0, 2, 1, 3)) for which in (0, 1)]
    out = guarded((B, N, C), torch.bfloat16)
    # K and V each in their own poisoned allocation (an over-read of K must not land in V)
    _lib.check(sdlib.sd_op_attention_headmajor(stream(), P(q), C, P(guarded_input(kv[0])), P(guarded_input(kv[1])), P(out), C, B, H,
                                               N, N, D, 1.0 / math.sqrt(D)))
    torch.cuda.synchronize()
    qh = q.float().cpu().view(B, N, H, D).transpose(1, 2)
    ref = F.scaled_dot_product_attention(qh, kv[0].float().cpu(), kv[1].float().cpu()).transpose(1, 2).reshape(B, N, C)
    ea = rel_l2(out, ref)
    print(f"head-major q|k|v B={B} tokens={N}: q {eq:.3e} k {ekv[0]:.3e} v {ekv[1]:.3e}, attention {ea:.3e}")
    assert eq < OP_TOL and max(ekv) < OP_TOL and ea < ATTN_TOL
    r64, b64 = gemm_bound(x, w)
    assert_elementwise(q, r64[:, :C], b64[:, :C], f"gemm qkv head-major q B={B} N={N}", ("row", "col"))
    for which in (0, 1):
        sl = slice((1 + which) * C, (2 + which) * C)
        hm = lambda t: t[:, sl].reshape(B, N, H, D).permute(0, 2, 1, 3)
        assert_elementwise(kv[which], hm(r64), hm(b64), f"gemm qkv head-major {'kv'[which]} B={B} N={N}", ("b", "head", "token", "d"))
    # the token-major call on the same data gives the same result bit for bit
    ktm = kv[0].permute(0, 2, 1, 3).reshape(B, N, C).contiguous()
    vtm = kv[1].permute(0, 2, 1, 3).reshape(B, N, C).contiguous()
    out2 = guarded(out.shape, out.dtype)
    _lib.check(sdlib.sd_op_attention(stream(), P(q), C, P(ktm), C, P(vtm), C, P(out2), C, B, H, N, N, D, 1.0 / math.sqrt(D)))
    torch.cuda.synchronize()
    assert torch.equal(out, out2)
    attention_elementwise(out, q.view(B, N, C), ktm, vtm, H, D, f"attention head-major B={B} N={N}")


def fold_layernorm(w, gamma, beta, bias):
    """Host-side packing of a LayerNorm-folded GEMM weight (test_ops_gpu.py)."""
    wg = r16(w * gamma[None, :])
    c1 = wg.double().sum(1).float()
    c2 = (w.double() @ beta.double()).float() + (bias if bias is not None else 0.0)
    return wg, c1, c2


def _gemm_plan(sdlib, x, w, bias, M, N, K, ln, hm_tokens=0):
    ncols = N // 3 if hm_tokens else N
    out = guarded((M, ncols), torch.bfloat16)
    kv = (guarded((2, M // hm_tokens, ncols // 40, hm_tokens, 40), torch.bfloat16)
          if hm_tokens else None)
    ln_rs, ln_parts, ln_c1 = ln
    _lib.check(sdlib.sd_op_gemm_plan(stream(), P(x), K, None, 0, K, P(w), P(bias), None, None, N, P(out), ncols, M, N, K,
                                     None, None, P(ln_rs), ln_parts, P(ln_c1), 1e-5, P(kv), hm_tokens))
    torch.cuda.synchronize()
    return out, kv


@pytest.mark.parametrize("B,tokens", [(3, 3840), (6, 1536)])
def test_gemm_plan_layernorm_fold_with_head_major_kv_at_non_power_of_two_tokens(sdlib, B, tokens):
    """norm1 folded into the q|k|v projection AND K / V stored head-major, as the plan runs a 48x80-latent batch's 64x64-
    equivalent level (3840 tokens) -- on the general kernel (not a power of two).  Against LayerNorm + linear, and its
    head-major K / V are exactly the token-major columns of the same call without the option."""
    C = 320
    M, N = B * tokens, 3 * C
    g = torch.Generator().manual_seed(B + tokens)
    h = r16(torch.randn(M, C, generator=g) * 2 + 0.3)
    h[:, 3] += 9.0
    gamma, beta = torch.randn(C, generator=g), torch.randn(C, generator=g)
    w = torch.randn(N, C, generator=g) / math.sqrt(C)
    wg, c1, c2 = fold_layernorm(w, gamma, beta, torch.zeros(N))
    parts = 2 * (C // 160)
    hh = h.view(M, parts, C // parts)
    rs = torch.stack([hh.sum(2), (hh * hh).sum(2)], dim=2).permute(1, 0, 2).contiguous()
    ln = (rs.cuda(), parts, c1.cuda())
    xd, wd, c2d = h.to("cuda", torch.bfloat16), wg.to("cuda", torch.bfloat16), c2.cuda()
    plain, _ = _gemm_plan(sdlib, xd, wd, c2d, M, N, C, ln)
    ref = F.layer_norm(h, (C,), gamma, beta, 1e-5) @ r16(w).t()
    err = rel_l2(plain, ref)
    q, kv = _gemm_plan(sdlib, xd, wd, c2d, M, N, C, ln, hm_tokens=tokens)
    print(f"LayerNorm-fold q|k|v, head-major K / V, B={B} tokens={tokens}: rel-L2 {err:.3e}")
    assert err < OP_TOL
    ln_fold_elementwise(plain, h, wg, c1, c2, rs, 0, f"gemm plan ln-fold B={B} tokens={tokens}")
    assert torch.equal(q, plain[:, :C])
    for which in (0, 1):
        want = plain[:, (1 + which) * C:(2 + which) * C].reshape(B, tokens, C // 40, 40).permute(0, 2, 1, 3)
        assert torch.equal(kv[which], want)


# ------------------------------------------------------------------------------------------ cross-attention forms
def _xattn_operands(g, B, hw, C, L=77, H=8):
    """Prompt K / V, the folded operands A^T (scale K_h W_q,h) / B (V_h W_o,h^T) and their tiled layouts (test_ops_gpu.py)."""
    d = C // H
    wq, wo = (torch.randn(C, C, generator=g) / math.sqrt(C) for _ in range(2))
    wk, wv = (torch.randn(C, 768, generator=g) / math.sqrt(768) for _ in range(2))
    bo = torch.randn(C, generator=g)
    ctx = torch.randn(B, L, 768, generator=g)
    ctx[0, 5] *= 4.0
    K, V = ctx @ wk.t(), ctx @ wv.t()
    scale = 1.0 / math.sqrt(d)
    At = torch.zeros(B, H * 80, C, dtype=torch.float64)
    Bn = torch.zeros(B, H * 80, C)
    for hh in range(H):
        sl = slice(hh * d, (hh + 1) * d)
        At[:, hh * 80: hh * 80 + L] = (scale * K[:, :, sl] @ wq[sl, :]).double()
        Bn[:, hh * 80: hh * 80 + L] = V[:, :, sl] @ wo[:, sl].t()
    return dict(wq=wq, wo=wo, bo=bo, K=K, V=V, At=At, Bn=r16(Bn), H=H, d=d, L=L)


def _tile_xattn(At, Bn, B, C, H=8):
    slot = torch.arange(H * 80)
    perm = (slot & ~12) | ((slot & 4) << 1) | ((slot & 8) >> 1)
    Bw = torch.zeros(B, C, H * 80)
    Bw[:, :, perm] = Bn.transpose(1, 2)
    At_t = At.float().view(B, H * 80, C // 32, 32).permute(0, 2, 1, 3).contiguous()
    Bw_t = Bw.view(B, C // 32, 32, 20, 32).permute(0, 1, 3, 2, 4).contiguous()
    return At_t, Bw_t


def _sdpa_xattn(o, xn, r, B, hw, C):
    q = (xn @ o["wq"].t()).view(B, hw, o["H"], o["d"]).transpose(1, 2)
    kk, vv = (t.view(B, o["L"], o["H"], o["d"]).transpose(1, 2) for t in (o["K"], o["V"]))
    a = F.scaled_dot_product_attention(q, kk, vv).transpose(1, 2).reshape(B, hw, C)
    return (r.view(B, hw, C) + a @ o["wo"].t() + o["bo"]).view(B * hw, C)


# rows per sample that are multiples of 128 but not powers of two (the fused form's rows_per_sample): 1536 (level 1 of a
# 64x96 latent: C = 640; level 0 of 32x48), 3840 (level 0 of 48x80), 6144 (level 0 of 64x96)
XATTN_FUSED = [(2, 1536, 640), (2, 3840, 320), (1, 6144, 320)]


@pytest.mark.parametrize("B,hw,C", XATTN_FUSED)
def test_xattn_fused_at_non_power_of_two_rows_per_sample(sdlib, B, hw, C):
    g = torch.Generator().manual_seed(B * 1000 + hw + C)
    M = B * hw
    x = r16(torch.randn(M, C, generator=g))
    r = r16(torch.randn(M, C, generator=g))
    o = _xattn_operands(g, B, hw, C)
    At = r16(o["At"].float())
    S = torch.einsum("bmc,bkc->bmk", x.view(B, hw, C), At).view(B, hw, o["H"], 80)
    S[..., o["L"]:] = float("-inf")
    Pm = torch.softmax(S, dim=-1).view(B, hw, o["H"] * 80)
    ref_fold = (r.view(B, hw, C) + torch.einsum("bmk,bkc->bmc", Pm, o["Bn"]) + o["bo"]).view(M, C)
    ref_attn = _sdpa_xattn(o, x.view(B, hw, C), r, B, hw, C)
    At_t, Bw_t = _tile_xattn(At, o["Bn"], B, C)
    out = guarded((M, C), torch.bfloat16)
    _lib.check(sdlib.sd_op_xattn_fused(stream(), P(x, torch.bfloat16), P(r, torch.bfloat16), P(out), P(At_t, torch.bfloat16),
                                       P(Bw_t, torch.bfloat16), P(o["bo"]), M, C, hw, o["L"]))
    torch.cuda.synchronize()
    e1, e2 = rel_l2(out, ref_fold), rel_l2(out, ref_attn)
    print(f"xattn fused B={B} hw={hw} C={C}: vs folded fp32 {e1:.3e}, vs SDPA + linears {e2:.3e}")
    assert torch.isfinite(out.float()).all()
    assert e1 < 8e-3 and e2 < 2e-2               # test_ops_gpu.py::test_xattn_fused's gates
    sel = sample_rows(B, hw)
    x64, A64 = x.double().view(B, hw, C)[sel], At.double()[sel]
    xattn_elementwise(out.view(B, hw, C)[sel], torch.einsum("bmc,bkc->bmk", x64, A64), torch.einsum("bmc,bkc->bmk", x64.abs(), A64.abs()),
                      U32 * (C + 2), o["Bn"][sel], r.view(B, hw, C)[sel], o["bo"], o["L"], f"xattn fused B={B} hw={hw} C={C}")


@pytest.mark.parametrize("B,hw,C", XATTN_FUSED)
def test_xattn_fused_with_norm2_folded_at_non_power_of_two_rows_per_sample(sdlib, B, hw, C):
    g = torch.Generator().manual_seed(B * 1000 + hw + C + 7)
    M = B * hw
    x = r16(torch.randn(M, C, generator=g) * 0.7 + 0.8 + 0.3 * torch.randn(M, 1, generator=g))
    r = r16(torch.randn(M, C, generator=g))
    gamma, beta = 1.0 + 0.3 * torch.randn(C, generator=g), 0.3 * torch.randn(C, generator=g)
    o = _xattn_operands(g, B, hw, C)
    Ag = o["At"] * gamma.double()
    At_ln = r16((Ag - Ag.mean(-1, keepdim=True)).float())
    c2 = (o["At"] @ beta.double()).float().contiguous()
    parts = 2 * ((C + 159) // 160)
    xs64 = x.double().view(M, C // 80, 80)
    rs = torch.stack([xs64.sum(-1), (xs64 * xs64).sum(-1)], -1).permute(1, 0, 2).float().contiguous()
    mean = x.double().mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(x.double().var(-1, unbiased=False, keepdim=True) + 1e-5)
    S = (rstd * torch.einsum("bmc,bkc->bmk", x.double().view(B, hw, C), At_ln.double()).view(M, o["H"] * 80)
         + c2.double().repeat_interleave(hw, 0)).view(B, hw, o["H"], 80)
    S[..., o["L"]:] = float("-inf")
    Pm = torch.softmax(S, dim=-1).view(B, hw, o["H"] * 80).float()
    ref_fold = (r.view(B, hw, C) + torch.einsum("bmk,bkc->bmc", Pm, o["Bn"]) + o["bo"]).view(M, C)
    xn = (((x.double() - mean) * rstd) * gamma.double() + beta.double()).float().view(B, hw, C)
    ref_attn = _sdpa_xattn(o, xn, r, B, hw, C)
    At_t, Bw_t = _tile_xattn(At_ln, o["Bn"], B, C)
    out = guarded((M, C), torch.bfloat16)
    oparts = sdlib.sd_op_ln_partials(1, M, C)
    ors = guarded((oparts, M, 2), torch.float32)
    _lib.check(sdlib.sd_op_xattn_fused_ln(stream(), P(x, torch.bfloat16), P(r, torch.bfloat16), P(out), P(At_t, torch.bfloat16),
                                          P(Bw_t, torch.bfloat16), P(o["bo"]), M, C, hw, o["L"], P(rs), parts, M, P(c2), 1e-5, P(ors)))
    torch.cuda.synchronize()
    e1, e2 = rel_l2(out, ref_fold), rel_l2(out, ref_attn)
    print(f"xattn fused + norm2 B={B} hw={hw} C={C}: vs folded fp64 {e1:.3e}, vs LayerNorm + SDPA + linears {e2:.3e}")
    assert torch.isfinite(out.float()).all()
    assert e1 < 8e-3 and e2 < 2e-2
    xattn_norm2_elementwise(out, x, At_ln, c2, rs, o["Bn"], r, o["bo"], o["L"], B, hw, C, M,
                            f"xattn fused+norm2 B={B} hw={hw} C={C}")
    tot = ors.sum(0).cpu()
    assert torch.allclose(tot[:, 0].double(), out.double().cpu().sum(1), rtol=1e-4, atol=1e-2)


# rows per sample of the two-GEMM fold (<= 1024 tokens, multiples of 128): 384 (16x24, level 2 of 64x96), 640 (level 2 of
# 80x128 / level 1 of 40x64), 768 (level 2 of 96x128)
FOLD_ROWS = [(2, 384, 1280), (2, 640, 640), (2, 768, 1280)]


@pytest.mark.parametrize("B,rows,C", FOLD_ROWS)
def test_fold_gemms_at_non_power_of_two_rows_per_sample(sdlib, B, rows, C):
    """The two GEMMs of the folded prompt cross-attention (per-sample weights; P = softmax_77(X A) in the first epilogue,
    h2 = h1 + P B + b_o in the second) against the same formula in fp32 from the rounded operands, and the unfolded
    attention."""
    g = torch.Generator().manual_seed(B + rows + C)
    M, NP = B * rows, 640
    x = r16(torch.randn(M, C, generator=g))
    r = r16(torch.randn(M, C, generator=g))
    o = _xattn_operands(g, B, rows, C)
    At = r16(o["At"].float())                                                # [B, 640, C]
    S = torch.einsum("brk,bnk->brn", x.view(B, rows, C), At).view(B, rows, 8, 80)
    Pref = torch.zeros_like(S)
    Pref[..., :77] = torch.softmax(S[..., :77], dim=-1)
    Pref = Pref.view(M, NP)
    pd = guarded((M, NP), torch.bfloat16)
    _lib.check(sdlib.sd_op_gemm_batched(stream(), P(x, torch.bfloat16), C, P(At, torch.bfloat16), NP * C, rows, None, None, NP,
                                        P(pd), NP, M, NP, C, 2, 77))
    torch.cuda.synchronize()
    e1 = rel_l2(pd, Pref)
    s64 = torch.einsum("brk,bnk->brn", x.double().view(B, rows, C), At.double()).reshape(M, NP)
    m64 = torch.einsum("brk,bnk->brn", x.double().abs().view(B, rows, C), At.double().abs()).reshape(M, NP)
    grouped_softmax_elementwise(pd, s64, U32 * C * m64, 77, f"fold gemm softmax B={B} rows={rows} C={C}")
    po = pd.float().cpu().view(M, 8, 80)
    assert (po[..., 77:] == 0).all() and (po.sum(-1) - 1).abs().max() < 2e-2
    Bt = o["Bn"].transpose(1, 2).contiguous()                                # [B, C, 640]: per-sample W of the second GEMM
    out = guarded((M, C), torch.bfloat16)
    _lib.check(sdlib.sd_op_gemm_batched(stream(), P(pd), NP, P(Bt, torch.bfloat16), C * NP, rows, P(o["bo"]), P(r, torch.bfloat16), C,
                                        P(out), C, M, C, NP, 0, 0))
    torch.cuda.synchronize()
    ref2 = (r.view(B, rows, C) + torch.einsum("brk,bck->brc", po.view(B, rows, NP), Bt) + o["bo"]).view(M, C)
    pb, Bb = po.double().view(B, rows, NP), r16(Bt).double()               # from the kernel's own stored P
    r64 = (torch.einsum("brk,bck->brc", pb, Bb) + r.double().view(B, rows, C) + o["bo"].double()).view(M, C)
    m64 = (torch.einsum("brk,bck->brc", pb.abs(), Bb.abs()) + r.double().abs().view(B, rows, C) + o["bo"].double().abs()).view(M, C)
    assert_elementwise(out, r64, linear_bound(r64, m64, NP + 2), f"fold gemm P B + R B={B} rows={rows} C={C}", ("row", "col"))
    e2 = rel_l2(out, ref2)
    e3 = rel_l2(out, _sdpa_xattn(o, x.view(B, rows, C), r, B, rows, C))
    print(f"fold GEMMs B={B} rows={rows} C={C}: P {e1:.3e}, P B + R {e2:.3e}, vs SDPA + linears {e3:.3e}")
    assert e1 < OP_TOL and e2 < OP_TOL and e3 < 2e-2


@pytest.mark.parametrize("B,rows,C", FOLD_ROWS)
def test_fold_softmax_gemm_with_norm2_at_non_power_of_two_rows_per_sample(sdlib, B, rows, C):
    """The first fold GEMM with norm2 folded in (sd_op_gemm_batched_softmax_ln) against LayerNorm + einsum + softmax in fp64
    (test_ops_gpu.py::test_gemm_per_sample_softmax_with_layernorm_folded's gate)."""
    g = torch.Generator().manual_seed(rows + C + 3)
    N, L, M = 640, 77, B * rows
    x = r16(torch.randn(M, C, generator=g) * 0.8 + 0.6)
    gamma, beta = 1.0 + 0.3 * torch.randn(C, generator=g), 0.3 * torch.randn(C, generator=g)
    w = (torch.randn(B, N, C, generator=g) / math.sqrt(C) * 3.0).double()
    wg = w * gamma.double()
    wln = r16((wg - wg.mean(-1, keepdim=True)).float())
    c1 = wln.double().sum(-1).float().contiguous()
    c2 = (w @ beta.double()).float().contiguous()
    parts = 2 * ((C + 159) // 160)
    xs = x.double().view(M, C // 80, 80)
    rs = torch.stack([xs.sum(-1), (xs * xs).sum(-1)], -1).permute(1, 0, 2).float().contiguous()
    mean = x.double().mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(x.double().var(-1, unbiased=False, keepdim=True) + 1e-5)
    xn = ((x.double() - mean) * rstd * gamma.double() + beta.double()).view(B, rows, C)
    S = torch.einsum("brk,bnk->brn", xn, w).view(B, rows, N // 80, 80)
    ref = torch.zeros_like(S)
    ref[..., :L] = torch.softmax(S[..., :L], dim=-1)
    ref = ref.view(M, N).float()
    out = guarded((M, N), torch.bfloat16)
    _lib.check(sdlib.sd_op_gemm_batched_softmax_ln(stream(), P(x, torch.bfloat16), C, P(wln, torch.bfloat16), N * C, rows, P(out), N,
                                                   M, N, C, L, P(rs), parts, P(c1), P(c2), 1e-5))
    torch.cuda.synchronize()
    e = rel_l2(out, ref)
    print(f"softmax GEMM + norm2 B={B} rows={rows} C={C}: rel-L2 {e:.3e}")
    assert e < 1e-2
    tot = rs.double().sum(0)
    zs, dzs = zip(*(ln_fold_ref_bound(x[b * rows:(b + 1) * rows], wln[b], c1[b], c2[b], tot[b * rows:(b + 1) * rows, 0],
                                      tot[b * rows:(b + 1) * rows, 1], 1e-5) for b in range(B)))
    grouped_softmax_elementwise(out, torch.cat(zs), torch.cat(dzs), L, f"fold softmax+ln B={B} rows={rows} C={C}")
    o = out.float().view(M, N // 80, 80)
    assert (o[..., L:] == 0).all() and (o.sum(-1) - 1).abs().max() < 2e-2


@pytest.mark.parametrize("M,C", [(2 * 25, 1280), (2 * 140, 1280), (2 * 1600, 320), (2 * 2240, 320)])
def test_to_q_gemm_with_norm2_folded_at_ragged_row_counts(sdlib, M, C):
    """Cross-attention "mode 2" (neither fused form applies: 25 / 140 / 1600 / 2240 tokens per sample): to_q runs as
    sd_op_gemm_ln on the un-normalised rows with norm2 folded in.  M is not a multiple of the 64- or 128-row tile."""
    g = torch.Generator().manual_seed(M + C)
    h = r16(torch.randn(M, C, generator=g) * 2 + 0.7)
    h[:, 5] += 10.0
    gamma, beta = torch.randn(C, generator=g), torch.randn(C, generator=g)
    w = torch.randn(C, C, generator=g) / math.sqrt(C)
    wg, c1, c2 = fold_layernorm(w, gamma, beta, None)
    parts = 2 * ((C + 159) // 160)
    hh = h.double().view(M, parts, C // parts)
    rs = torch.stack([hh.sum(2), (hh * hh).sum(2)], dim=2).permute(1, 0, 2).float().contiguous()
    out = guarded((M, C), torch.bfloat16)
    _lib.check(sdlib.sd_op_gemm_ln(stream(), P(h, torch.bfloat16), C, P(wg, torch.bfloat16), P(c1), P(c2), P(rs), parts, 1e-5,
                                   P(out), C, M, C, C, 0))
    torch.cuda.synchronize()
    ref = F.layer_norm(h, (C,), gamma, beta, 1e-5) @ r16(w).t()
    err = rel_l2(out, ref)
    print(f"to_q + norm2 fold M={M} C={C}: rel-L2 {err:.3e}")
    assert torch.isfinite(out.float()).all() and err < OP_TOL
    ln_fold_elementwise(out, h, wg, c1, c2, rs, 0, f"to_q ln-fold M={M} C={C}")


# ------------------------------------------------------------------------------------------ GroupNorm
def _gn_case(sdlib, B, HW, C1, C2, silu, eps, seed):
    """Per element and by count (tests/bounds.py::assert_flip_budget, budget 4 F_ref + 8).  Measured flips / F_ref / numel --
    small kernel: 0 / 3 / 128000, 10 / 12 / 134400, 15 / 17 / 241920, 100 / 132 / 2867200, 7 / 15 / 358400, 28 / 52 / 645120,
    4 / 9 / 161280; split statistics: 13 / 34 / 512000, 34 / 99 / 1075200, 126 / 439 / 2580480, 443 / 1179 / 12288000,
    33 / 57 / 716800, 9 / 13 / 268800, 37 / 124 / 1024000, 175 / 874 / 4300800."""
    g = torch.Generator().manual_seed(seed)
    C = C1 + C2
    x = r16(torch.randn(B, HW, C, generator=g) * 2 + 0.5)
    gamma, beta = torch.randn(C, generator=g), torch.randn(C, generator=g)
    ref = F.group_norm(x.permute(0, 2, 1).double(), 32, gamma.double(), beta.double(), eps).float()
    if silu:
        ref = F.silu(ref)
    ref = ref.permute(0, 2, 1)
    out = guarded((B, HW, C), torch.bfloat16)
    _lib.check(sdlib.sd_op_groupnorm(stream(), P(x[..., :C1].contiguous(), torch.bfloat16), C1,
                                     P(x[..., C1:].contiguous(), torch.bfloat16) if C2 else None, C2, P(gamma), P(beta), P(out),
                                     B, HW, 32, eps, silu))
    torch.cuda.synchronize()
    n64, nb = norm_ref_bound(x, gamma, beta, HW * C // 32, eps, silu, groups=32)
    assert_elementwise(out, n64, nb, f"groupnorm odd pixels B={B} HW={HW} C={C1}+{C2}", ("b", "pixel", "c"))
    assert_flip_budget(out, n64, gn_restatements(x, gamma, beta, 32, eps, silu), "bf16",
                       f"groupnorm odd pixels B={B} HW={HW} C={C1}+{C2}", acc_bound=nb - ulp_bf16(n64))
    return rel_l2(out, ref)


# (B, HW, C1, C2): the deepest levels of the odd sizes -- 5x5, 5x7, 7x9, 10x14, 14x18 pixels.  <= 256 pixels and <= 10240
# values per group: the single-launch small kernel (csrc/norm.hip, sd_groupnorm_uses_small); concats of the up blocks with a
# group straddling the two sources (1280 + 640: groups of 60 channels, group 21 = channels 1260..1319)
@pytest.mark.parametrize("B,HW,C1,C2", [(2, 25, 1280, 1280), (2, 35, 1280, 640), (2, 63, 1280, 640), (32, 35, 1280, 1280),
                                        (2, 140, 1280, 0), (2, 252, 1280, 0), (2, 63, 1280, 0)])
def test_groupnorm_small_kernel_at_odd_pixel_counts(sdlib, B, HW, C1, C2):
    err = _gn_case(sdlib, B, HW, C1, C2, 1, 1e-5, HW + C1 + C2 + B)
    print(f"GroupNorm (small kernel) B={B} HW={HW} C={C1}+{C2}: rel-L2 {err:.3e}")
    assert err < OP_TOL


# the split-statistics path (> 256 pixels, or too many values per group for the small kernel) at pixel counts that are not
# multiples of 64: 400 / 560 / 1008 (level 1 of 40x40 / 40x56 / 56x72), 140 pixels x 2560 channels (a concat at 10x14: 80
# channels per group, 11200 values; 960 channels: 30 per group, not a multiple of 4), and 1600 / 2240 at level 0
@pytest.mark.parametrize("B,HW,C1,C2", [(2, 400, 640, 0), (2, 560, 640, 320), (2, 1008, 640, 640), (32, 400, 640, 320),
                                        (2, 140, 1280, 1280), (2, 140, 640, 320), (2, 1600, 320, 0), (2, 2240, 320, 640)])
def test_groupnorm_split_statistics_at_ragged_pixel_counts(sdlib, B, HW, C1, C2):
    err = _gn_case(sdlib, B, HW, C1, C2, 1, 1e-5, HW + C1 + C2 + B + 1)
    print(f"GroupNorm (split statistics) B={B} HW={HW} C={C1}+{C2}: rel-L2 {err:.3e}")
    assert err < OP_TOL


@pytest.mark.parametrize("B,H,W,Cin,Cout,res", [(2, 5, 5, 1280, 1280, True), (2, 5, 7, 1280, 1280, True), (2, 7, 9, 2560, 1280, False),
                                                (2, 10, 14, 1280, 1280, True), (32, 5, 7, 1280, 1280, True)])
def test_conv3x3_groupnorm_deferred_splitk_reduce_at_odd_sizes(sdlib, B, H, W, Cin, Cout, res):
    """The resnet conv -> GroupNorm pair at the deepest levels of 40x40 / 40x56 / 56x72 / 80x112-ish latents: a split-K conv
    leaves its fp32 slabs to the single-launch GroupNorm (gn_slab_kernel), which finishes the reduce at pixel counts that
    are not multiples of 32.  Against fp32 torch, and bit-identical to conv + reduce, then the GroupNorm (SD_GN_SLAB=0)."""
    g = torch.Generator().manual_seed(H * W + Cin + Cout + B)
    x = r16(torch.randn(B, Cin, H, W, generator=g))
    w = r16(torch.randn(Cout, Cin, 3, 3, generator=g) / math.sqrt(9 * Cin))
    b, b2 = torch.randn(Cout, generator=g), torch.randn(Cout, generator=g)
    r = r16(torch.randn(B, Cout, H, W, generator=g)) if res else None
    gamma, beta = torch.randn(Cout, generator=g), torch.randn(Cout, generator=g)
    conv = r16(F.conv2d(x, w, b, padding=1) + b2[None, :, None, None] + (r if res else 0.0))
    ref = F.silu(F.group_norm(conv, 32, gamma, beta, 1e-5))
    xd = x.permute(0, 2, 3, 1).contiguous().to("cuda", torch.bfloat16)
    wd = w.permute(0, 2, 3, 1).reshape(Cout, 9, Cin // 64, 64).permute(0, 2, 1, 3).contiguous().to("cuda", torch.bfloat16)
    rd = r.permute(0, 2, 3, 1).contiguous().to("cuda", torch.bfloat16) if res else None

    def run():
        y = guarded((B, H, W, Cout), torch.bfloat16)
        yn = guarded(y.shape, y.dtype)
        _lib.check(sdlib.sd_op_conv3x3_groupnorm(stream(), P(xd), P(wd), P(b), P(b2), P(rd), P(y), B, H, W, Cin, Cout,
                                                 P(gamma), P(beta), P(yn), 32, 1e-5, 1))
        torch.cuda.synchronize()
        return y, yn
    splitk = sdlib.sd_op_conv3x3_splitk(B * H * W, Cout, Cin, H, W, 1, 0)
    assert splitk > 1                                  # the case exists to exercise the slabs
    y, yn = run()
    e1, e2 = rel_l2(y.permute(0, 3, 1, 2), conv), rel_l2(yn.permute(0, 3, 1, 2), ref)
    y2, yn2 = env_once("SD_GN_SLAB", "0", run)
    print(f"conv -> GroupNorm {B}x{H}x{W} {Cin}->{Cout} split-K {splitk}: conv {e1:.3e}, norm {e2:.3e}")
    assert e1 < OP_TOL and e2 < OP_TOL
    assert torch.equal(y.view(torch.int16), y2.view(torch.int16))
    assert torch.equal(yn.view(torch.int16), yn2.view(torch.int16))
    conv_gn_elementwise(x, w, b, b2, r, gamma, beta, y, (yn,), f"conv3x3+gn split-K odd {B}x{H}x{W} {Cin}->{Cout}")


# ------------------------------------------------------------------------------------------ 3x3 conv
# (B, Hin, Win, Cin, Cout, upsample, kernel): stride-1 convs of the UNet levels of the odd sizes (widths 5, 7, 9, 14, 18,
# 20, 28, 36; the 4x16 / 16x4 deepest levels of 32x128 / 128x32) and fused upsamplers (nearest 2x + conv; the plan's form
# where the low-res pixels are not a multiple of 64), with the kernel sd_op_conv3x3_kernel reports: 1 = halo kernel (its
# geometry mode for non-power-of-two widths), 0 = implicit GEMM.  The table holds at least one shape of every
# (form, kernel, split-K > 1, power-of-two output width) class the legal sizes produce at UNet batch 2 and 32
# (tests/test_resolution_cpu.py::test_edge_conv_table_covers_every_kernel_class).
EDGE_CONV_SHAPES = [
    (2, 5, 5, 1280, 1280, 0, 0), (2, 5, 7, 1280, 1280, 0, 0), (2, 7, 9, 1280, 1280, 0, 0), (2, 10, 14, 1280, 1280, 0, 0),
    (2, 14, 18, 1280, 1280, 0, 1), (2, 20, 20, 640, 640, 0, 1), (2, 20, 28, 640, 640, 0, 1), (2, 28, 36, 640, 640, 0, 1),
    (2, 4, 16, 1280, 1280, 0, 0), (2, 16, 4, 1280, 1280, 0, 0), (2, 7, 9, 2560, 1280, 0, 0), (2, 8, 32, 1280, 1280, 0, 1),
    (2, 32, 40, 320, 320, 0, 1), (2, 32, 32, 320, 320, 0, 1),
    (32, 7, 9, 1280, 1280, 0, 0), (32, 14, 18, 640, 640, 0, 1), (32, 32, 40, 320, 320, 0, 1), (32, 32, 32, 320, 320, 0, 1),
    (32, 32, 80, 320, 160, 0, 0), (32, 32, 128, 320, 160, 0, 0),
    (2, 5, 7, 1280, 1280, 1, 0), (2, 7, 9, 1280, 1280, 1, 1), (2, 5, 4, 1280, 1280, 1, 0), (2, 8, 10, 1280, 1280, 1, 1),
    (2, 4, 4, 1280, 1280, 1, 1), (32, 8, 22, 640, 640, 1, 0), (32, 8, 10, 1280, 1280, 1, 1), (32, 10, 8, 1280, 1280, 1, 1),
]


def _conv_ref(x, w, b, up, stride=1):
    xin = F.interpolate(x, scale_factor=2.0, mode="nearest") if up else x
    return F.conv2d(xin, w, b, stride=stride, padding=1)


def _pack_w(w):
    Cout, Cin = w.shape[:2]
    return w.permute(0, 2, 3, 1).reshape(Cout, 9, Cin // 64, 64).permute(0, 2, 1, 3).contiguous()


@pytest.mark.parametrize("B,H,W,Cin,Cout,up,kernel", EDGE_CONV_SHAPES)
def test_conv3x3_at_odd_level_sizes_bf16(sdlib, B, H, W, Cin, Cout, up, kernel):
    g = torch.Generator().manual_seed(B * 1000 + H * 10 + W + Cin + up)
    x = r16(torch.randn(B, Cin, H, W, generator=g))
    w = r16(torch.randn(Cout, Cin, 3, 3, generator=g) / math.sqrt(9 * Cin))
    b, b2 = torch.randn(Cout, generator=g), torch.randn(Cout, generator=g)
    ref = _conv_ref(x, w, b, up) + b2[None, :, None, None]
    Ho, Wo = ref.shape[-2:]
    r = r16(torch.randn(B, Cout, Ho, Wo, generator=g))
    ref = ref + r
    out = guarded((B, Ho, Wo, Cout), torch.bfloat16)
    _lib.check(sdlib.sd_op_conv3x3(stream(), P(x.permute(0, 2, 3, 1).contiguous(), torch.bfloat16), P(_pack_w(w), torch.bfloat16),
                                   P(b), P(b2), P(r.permute(0, 2, 3, 1).contiguous(), torch.bfloat16), P(out), B, H, W, Cin, Cout, 1, up))
    torch.cuda.synchronize()
    err = rel_l2(out.permute(0, 3, 1, 2), ref)
    kern = sdlib.sd_op_conv3x3_kernel(B * Ho * Wo, Cout, Cin, H, W, 1, up, 0)
    splitk = sdlib.sd_op_conv3x3_splitk(B * Ho * Wo, Cout, Cin, H, W, 1, up)
    print(f"conv3x3 {B}x{H}x{W} up={up} {Cin}->{Cout}: kernel {kern} split-K {splitk} rel-L2 {err:.3e}")
    assert kern == kernel and err < OP_TOL
    r64, m64 = conv3x3_nhwc_ref(x, w, b, b2, r, 1, up)
    assert_elementwise(out, r64, linear_bound(r64, m64, 9 * Cin + 3), f"conv3x3 odd {B}x{H}x{W} up{up} {Cin}->{Cout} k{kern} s{splitk}", NHWC)


@pytest.mark.parametrize("B,H,W,C", [(2, 10, 14, 1280), (2, 14, 18, 1280), (2, 20, 28, 640), (32, 10, 14, 1280)])
def test_conv3x3_stride2_from_odd_sizes(sdlib, B, H, W, C):
    """The downsamplers into the 5x7 / 7x9 / 10x14 levels (stride 2: always the implicit-GEMM kernel)."""
    g = torch.Generator().manual_seed(B + H * W + C)
    x = r16(torch.randn(B, C, H, W, generator=g))
    w = r16(torch.randn(C, C, 3, 3, generator=g) / math.sqrt(9 * C))
    b = torch.randn(C, generator=g)
    ref = _conv_ref(x, w, b, 0, stride=2)
    Ho, Wo = ref.shape[-2:]
    out = guarded((B, Ho, Wo, C), torch.bfloat16)
    _lib.check(sdlib.sd_op_conv3x3(stream(), P(x.permute(0, 2, 3, 1).contiguous(), torch.bfloat16), P(_pack_w(w), torch.bfloat16),
                                   P(b), None, None, P(out), B, H, W, C, C, 2, 0))
    torch.cuda.synchronize()
    err = rel_l2(out.permute(0, 3, 1, 2), ref)
    kern = sdlib.sd_op_conv3x3_kernel(B * Ho * Wo, C, C, H, W, 2, 0, 0)
    print(f"conv3x3 stride 2 {B}x{H}x{W} -> {Ho}x{Wo} C={C}: kernel {kern} rel-L2 {err:.3e}")
    assert kern == 0 and err < OP_TOL
    r64, m64 = conv3x3_nhwc_ref(x, w, b, None, None, 2)
    assert_elementwise(out, r64, linear_bound(r64, m64, 9 * C + 1), f"conv3x3 stride2 odd {B}x{H}x{W} C={C}", NHWC)


# fp8 (Cin a multiple of 128; the UNet's level-0 convs pad 320 to 384 and are covered at 64x96 by test_resolution_gpu.py)
EDGE_CONV_FP8 = [(2, 5, 7, 1280, 1280, 0, 0), (2, 7, 9, 1280, 1280, 0, 0), (2, 14, 18, 1280, 1280, 0, 1),
                 (2, 20, 28, 640, 640, 0, 1), (2, 28, 36, 640, 640, 0, 1), (2, 4, 16, 1280, 1280, 0, 0),
                 (2, 16, 4, 1280, 1280, 0, 0), (2, 5, 7, 1280, 1280, 1, 0), (2, 7, 9, 1280, 1280, 1, 1)]


@pytest.mark.parametrize("B,H,W,Cin,Cout,up,kernel", EDGE_CONV_FP8)
def test_conv3x3_at_odd_level_sizes_fp8(sdlib, B, H, W, Cin, Cout, up, kernel):
    from oracle.fp8 import quantize_rows
    g = torch.Generator().manual_seed(B * 100 + H + W + Cin + up)
    xs = 8.0
    xq = (torch.randn(B, Cin, H, W, generator=g) * xs).clamp(-448, 448).to(torch.float8_e4m3fn)
    wq, wsc = quantize_rows(torch.randn(Cout, Cin, 3, 3, generator=g) / math.sqrt(9 * Cin))
    wc = wq.clamp(-448, 448).to(torch.float8_e4m3fn).view(torch.uint8)
    b = torch.randn(Cout, generator=g)
    ref = _conv_ref(xq.float() / xs, wq * wsc[:, None, None, None], b, up)
    Ho, Wo = ref.shape[-2:]
    xd = xq.view(torch.uint8).permute(0, 2, 3, 1).contiguous()
    wd = wc.permute(0, 2, 3, 1).reshape(Cout, 9, Cin // 128, 128).permute(0, 2, 1, 3).contiguous()
    out = guarded((B, Ho, Wo, Cout), torch.bfloat16)
    _lib.check(sdlib.sd_op_conv3x3_fp8(stream(), P(xd), P(wd), P(wsc), xs, P(b), None, None, P(out), B, H, W, Cin, Cout, 1, up))
    torch.cuda.synchronize()
    err = rel_l2(out.permute(0, 3, 1, 2), ref)
    kern = sdlib.sd_op_conv3x3_kernel(B * Ho * Wo, Cout, Cin, H, W, 1, up, 1)
    print(f"conv3x3 fp8 {B}x{H}x{W} up={up} Cin={Cin}: kernel {kern} rel-L2 {err:.3e}")
    assert kern == kernel and err < OP_TOL
    r64, m64, k_eff = fp8_conv_ref(xq.float() / xs, wq, wsc, b, up=up)
    assert_elementwise(out, r64, linear_bound(r64, m64, k_eff), f"conv3x3 fp8 odd {B}x{H}x{W} up{up} {Cin}->{Cout} k{kern}", NHWC)


# ------------------------------------------------------------------------------------------ softmax rows
@pytest.mark.parametrize("rows,cols", [(7, 1600), (64, 1600), (5, 2240), (33, 3136)])
def test_softmax_rows_at_vae_mid_block_widths(sdlib, rows, cols):
    """The VAE mid-block attention's softmax at 40x40 / 40x56 / 56x56 latents: one wave per row (<= 4096 columns), widths
    that are not multiples of 512; a dominant score near the end of every row."""
    g = torch.Generator().manual_seed(cols + rows)
    s = r16(torch.randn(rows, cols, generator=g) * 20)
    s[:, cols - 3] = 400.0
    s[::2, cols - 9] = 420.0
    scale = 1 / math.sqrt(512)
    ref = torch.softmax(s * scale, dim=-1)
    d = guarded_input(s, torch.bfloat16)         # in place: the scores' own poisoned guards
    _lib.check(sdlib.sd_op_softmax_rows(stream(), d.data_ptr(), rows, cols, scale))
    torch.cuda.synchronize()
    err = rel_l2(d, ref)
    print(f"softmax {rows}x{cols}: rel-L2 {err:.3e}")
    assert torch.isfinite(d.float()).all() and err < OP_TOL
    assert torch.allclose(d.float().sum(-1).cpu(), torch.ones(rows), atol=2e-2)
    softmax_rows_elementwise(d, s, scale, f"softmax mid-block rows {rows}x{cols}")


# ------------------------------------------------------------------------------------------ large operands
# (B, H, W, Cin, Cout, kernel): inputs of 2^31 bytes and of 2^32 bytes.  The halo kernel addresses X through a buffer
# resource with 32-bit byte offsets (csrc/conv_halo.hip), so it refuses inputs of >= 2^32 bytes; and its halo slots limit it
# to images <= 64 pixels wide, so the 2^31-byte halo case is 256 64x64 images.  The VAE decoder's own large convs (512x512 x
# 512 channels at 8 images of 1024x1024 = 2^31 bytes, 1024x1024 x 256 channels = 2^32 bytes) are too wide for it and run on
# the implicit-GEMM kernel (64-bit row pointers).
LARGE_CONVS = [(256, 64, 64, 1024, 160, 1), (512, 64, 64, 1024, 160, 0), (8, 512, 512, 512, 512, 0), (8, 1024, 1024, 256, 128, 0)]


@pytest.mark.parametrize("B,H,W,Cin,Cout,kernel", LARGE_CONVS)
def test_conv3x3_large_operands(sdlib, B, H, W, Cin, Cout, kernel):
    """Device memory: the input (B H W Cin 2 bytes: 2 / 4 / 2 / 4 GiB) and the output (0.3 / 0.6 / 2 / 2 GiB) -- at most
    6 GiB.  Only the last image's last rows (the largest offsets) are checked against F.conv2d on the cropped input with
    its halo row above; the whole output must be finite."""
    nbytes = B * H * W * Cin * 2
    assert (1 << 31) <= nbytes
    assert sdlib.sd_op_conv3x3_kernel(B * H * W, Cout, Cin, H, W, 1, 0, 0) == kernel
    g = torch.Generator(device="cuda").manual_seed(B + H + Cin)
    x = torch.randn((B, H, W, Cin), generator=g, device="cuda", dtype=torch.bfloat16)
    w = (torch.randn((Cout, Cin, 3, 3), generator=g, device="cuda") / math.sqrt(9 * Cin)).to(torch.bfloat16).float()
    b = torch.randn(Cout, generator=g, device="cuda")
    wd = _pack_w(w).to(torch.bfloat16)
    out = torch.full((B, H, W, Cout), float("nan"), device="cuda", dtype=torch.bfloat16)     # no guards: device memory
    try:
        _lib.check(sdlib.sd_op_conv3x3(stream(), x.data_ptr(), wd.data_ptr(), b.data_ptr(), None, None,
                                       out.data_ptr(), B, H, W, Cin, Cout, 1, 0))
        torch.cuda.synchronize()
        R = 2
        crop = x[B - 1, H - R - 1:].float().cpu().permute(2, 0, 1)[None]              # [1, Cin, R + 1, W]
        ref = F.conv2d(F.pad(crop, (1, 1, 0, 1)), w.cpu(), b.cpu())                   # last R output rows of the last image
        got = out[B - 1, H - R:].float().cpu().permute(2, 0, 1)[None]
        err = rel_l2(got, ref)
        finite = bool(torch.isfinite(out).all())
        print(f"conv3x3 {B}x{H}x{W} {Cin}->{Cout} ({nbytes / 2**30:.1f} GiB input): kernel {kernel}, last rows rel-L2 {err:.3e}")
        assert finite and err < OP_TOL
        cp = F.pad(crop.double(), (1, 1, 0, 1))
        r64 = (F.conv2d(cp, w.cpu().double()) + b.cpu().double()[None, :, None, None]).permute(0, 2, 3, 1)
        m64 = (F.conv2d(cp.abs(), w.cpu().double().abs()) + b.cpu().double().abs()[None, :, None, None]).permute(0, 2, 3, 1)
        assert_elementwise(got.permute(0, 2, 3, 1), r64, linear_bound(r64, m64, 9 * Cin + 1),
                           f"conv3x3 large operands {B}x{H}x{W} {Cin}->{Cout} last rows", NHWC)
    finally:
        del x, wd, out
        torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------ UNet forward
_ORACLE = {}


@pytest.fixture(scope="module")
def sd15():
    from sonicdiffusionbayeslab_amd.weights import UNetConfig, make_synthetic_state_dict
    cfg = UNetConfig(sample_size=64)
    return cfg, make_synthetic_state_dict(cfg, seed=1234)


@pytest.fixture(scope="module")
def sd15_net(sd15):
    from sonicdiffusionbayeslab_amd.unet import HipUNet2DConditionModel
    cfg, sd = sd15
    net = HipUNet2DConditionModel(cfg, sd)
    yield net
    del net
    torch.cuda.empty_cache()


def inputs(latent_batch, h, w, seed, context_len=77, dim=768):
    g = torch.Generator().manual_seed(seed)
    lat = torch.randn((latent_batch, 4, h, w), generator=g)
    pe = torch.randn((latent_batch, context_len, dim), generator=g)
    ne = torch.randn((1, context_len, dim), generator=g).repeat(latent_batch, 1, 1)
    return lat, pe, ne


def _unet_oracle(sd15, h, w, t, seed):
    """fp32 CPU oracle of one CFG forward (latent batch 1 -> UNet batch 2), cached per case (the fp8 test reuses it)."""
    from oracle.unet import unet_forward
    key = (h, w, t, seed)
    if key not in _ORACLE:
        cfg, sd = sd15
        lat, pe, ne = inputs(1, h, w, seed)
        with torch.no_grad():
            _ORACLE[key] = unet_forward(sd, oracle_cfg(cfg), torch.cat([lat, lat]), t, torch.cat([ne, pe]))
    return _ORACLE[key]


@pytest.mark.parametrize("h,w,t", [(40, 40, 981.0), (40, 56, 981.0), (40, 56, 21.0), (56, 72, 501.0), (48, 80, 981.0),
                                   (32, 128, 981.0), (128, 32, 501.0), (128, 128, 981.0)])
def test_sd15_unet_cfg_forward_at_odd_sizes(sd15, sd15_net, h, w, t):
    """SD-1.5-shaped UNet, one CFG forward (UNet batch 2: the CFG-dedup plan) at 320x320, 320x448, 448x576, 384x640,
    256x1024, 1024x256 and 1024x1024 against the fp32 oracle.  The oracle at 128x128 costs ~16 s on 8 host cores."""
    seed = h * 1000 + w
    lat, pe, ne = inputs(1, h, w, seed)
    ctx = torch.cat([ne, pe])
    sd15_net.set_deepcache(-1)
    sd15_net.set_context(ctx.cuda(), h, w)
    eps = sd15_net.forward_latents(lat.cuda(), 2, t).cpu()
    ref = _unet_oracle(sd15, h, w, t, seed)
    err = rel_l2(eps, ref)
    print(f"SD-1.5 UNet {h}x{w} t={t}: rel-L2 {err:.3e} cos {cosine(eps, ref):.5f}")
    assert eps.shape == (2, 4, h, w) and torch.isfinite(eps).all() and err < UNET_TOL


@pytest.mark.parametrize("t", [981.0])
def test_sd15_unet_fp8_forward_at_40x56_matches_emulating_oracle(sd15, t):
    """fp8 weights at 320x448 against the oracle that emulates the fp8 scheme (test_fp8_gpu.py's gates: FWD_TOL against it,
    at most FWD_EXCESS times its own distance from the unquantised oracle, + 1e-2)."""
    from oracle.fp8 import Fp8Emulation
    from oracle.unet import unet_forward
    from sonicdiffusionbayeslab_amd.unet import HipUNet2DConditionModel
    FWD_TOL, FWD_EXCESS = 1.5e-1, 1.25
    cfg, sd = sd15
    h, w = 40, 56
    seed = h * 1000 + w
    net = HipUNet2DConditionModel(cfg, sd, weight_dtype="fp8")
    assert net.weight_dtype == "fp8_e4m3"
    lat, pe, ne = inputs(1, h, w, seed)
    ctx = torch.cat([ne, pe])
    net.set_context(ctx.cuda(), h, w)
    eps = net.forward_latents(lat.cuda(), 2, t).cpu()
    del net
    with torch.no_grad():
        ref_q = unet_forward(sd, oracle_cfg(cfg), torch.cat([lat, lat]), t, ctx, fq=Fp8Emulation(sd))
    ref = _unet_oracle(sd15, h, w, t, seed)
    e_q, e_f, e_o = rel_l2(eps, ref_q), rel_l2(eps, ref), rel_l2(ref_q, ref)
    print(f"fp8 UNet 40x56 t={t}: vs emulating oracle {e_q:.3e} (cos {cosine(eps, ref_q):.5f}); vs unquantised {e_f:.3e}; "
          f"oracle fp8-vs-fp32 {e_o:.3e}")
    assert torch.isfinite(eps).all()
    assert e_q < FWD_TOL and cosine(eps, ref) > 0.99
    assert e_f < FWD_EXCESS * e_o + 1e-2


# ------------------------------------------------------------------------------------------ VAE decoder
@pytest.fixture(scope="module")
def vae():
    from sonicdiffusionbayeslab_amd.vae import HipVaeDecoder, VaeConfig, make_synthetic_vae_state_dict
    cfg = VaeConfig(sample_size=64)
    sd = make_synthetic_vae_state_dict(cfg)
    dec = HipVaeDecoder(cfg, sd)
    yield cfg, sd, dec
    del dec
    torch.cuda.empty_cache()


@pytest.mark.parametrize("h,w", [(40, 40), (64, 72), (128, 128)])
def test_vae_decode_at_odd_sizes_matches_oracle(vae, h, w):
    """1600 mid-block tokens (one query chunk, a 1600-column softmax), 4608 (chunks of 2048 / 2048 / 512 rows), 16384 (8
    chunks, the long-row softmax); test_vae_gpu.py's gate.  The oracle at 128x128 costs ~20 s on 8 host cores."""
    import dataclasses
    from oracle.vae import VaeConfig as OC, vae_decode
    cfg, sd, dec = vae
    lat = torch.randn(1, 4, h, w, generator=torch.Generator().manual_seed(h * w))
    inv = 1.0 / cfg.scaling_factor
    got = dec.decode(lat.cuda(), inv).cpu()
    with torch.no_grad():
        ref = vae_decode(sd, OC(**dataclasses.asdict(cfg)), lat * inv)
    err, cs = rel_l2(got, ref), cosine(got, ref)
    print(f"VAE decode {h}x{w} -> {8 * h}x{8 * w}: rel-L2 {err:.3e} cos {cs:.5f}")
    assert got.shape == (1, 3, 8 * h, 8 * w) and torch.isfinite(got).all()
    assert err < 2e-2 and cs > 0.999


def test_vae_decode_eight_1024px_images_in_one_chunk(vae):
    """decode() of 8 different 128x128 latents runs as ONE chunk of 8 (its default), with activations of 2^31 and 2^32 bytes
    at the 512x512 and 1024x1024 levels (workspace ~11 GiB); every image against a 1-image decode of the same latent.  At
    this size every kernel choice of the decoder is the same for 1 and 8 images (measured: all 8 bit-identical), so the
    gate is torch.equal: an addressing error past 2^31 / 2^32 bytes in one image of the batch shows as a difference."""
    cfg, sd, dec = vae
    lat = torch.randn(8, 4, 128, 128, generator=torch.Generator().manual_seed(88))
    inv = 1.0 / cfg.scaling_factor
    ws8 = dec._lib.sd_unet_workspace_bytes_hw(dec._handle, 8, -1, 128, 128)
    got = dec.decode(lat.cuda(), inv).cpu()
    dec._ws = None
    torch.cuda.empty_cache()
    errs, same = [], 0
    for i in range(8):
        one = dec.decode(lat[i:i + 1].cuda(), inv).cpu()
        same += int(torch.equal(one, got[i:i + 1]))
        errs.append(rel_l2(got[i:i + 1], one))
    dec._ws = None
    torch.cuda.empty_cache()
    print(f"VAE decode 8 x 1024x1024 in one chunk (workspace {ws8 / 2**30:.1f} GiB): {same} of 8 bit-identical to 1-image "
          f"decodes, worst rel-L2 {max(errs):.3e}")
    assert torch.isfinite(got).all() and same == 8


# ------------------------------------------------------------------------------------------ pipeline
def test_pipeline_320x448_ddim_cfg_and_deepcache(sd15):
    """One DDIM loop (3 steps, CFG) at 320x448 through the pipeline, then the same with DeepCache (interval 3: steps 2 and 3
    run the cached branch), against oracle.pipeline.sample_loop."""
    from oracle.pipeline import sample_loop
    from oracle.schedulers import DDIMOracle
    from oracle.unet import DeepCacheState
    from sonicdiffusionbayeslab_amd.deepcache import DeepCacheSDHelper
    from sonicdiffusionbayeslab_amd.models import StableDiffusionModel
    from sonicdiffusionbayeslab_amd.registry import schedulers_registry
    from sonicdiffusionbayeslab_amd.schedulers import PNDMConfigStub
    cfg, sd = sd15
    pipe = StableDiffusionModel(unet_config=cfg, state_dict=dict(sd)).to("cuda:0")
    pipe.scheduler = schedulers_registry["ddim_scheduler"].from_config(PNDMConfigStub().config)
    lat, pe, ne = inputs(1, 40, 56, seed=43)
    out, secs, _ = pipe(prompt_embeds=pe, negative_prompt_embeds=ne, latents=lat, num_inference_steps=3, guidance_scale=7.5,
                        output_type="latent", height=320, width=448)
    ref, _, _, _ = sample_loop(sd, oracle_cfg(cfg), DDIMOracle(), pe, ne, lat, 3, 7.5)
    err, cs = rel_l2(out.images, ref), cosine(out.images, ref)
    print(f"DDIM 3 steps 320x448: rel-L2 {err:.3e} cos {cs:.5f}, loop {secs * 1e3:.1f} ms")
    assert out.images.shape == (1, 4, 40, 56) and err < FREE_TOL and cs > FREE_COS

    helper = DeepCacheSDHelper(pipe=pipe)
    helper.set_params(cache_interval=3, cache_branch_id=0)
    helper.enable()
    try:
        out, _, _ = pipe(prompt_embeds=pe, negative_prompt_embeds=ne, latents=lat, num_inference_steps=3,
                         guidance_scale=7.5, output_type="latent", height=320, width=448)
    finally:
        helper.disable()
    dc = DeepCacheState(cache_interval=3, cache_branch_id=0, enabled=True)
    ref, _, _, _ = sample_loop(sd, oracle_cfg(cfg), DDIMOracle(), pe, ne, lat, 3, 7.5, deepcache=dc)
    err, cs = rel_l2(out.images, ref), cosine(out.images, ref)
    print(f"DDIM 3 steps + DeepCache N=3 320x448: rel-L2 {err:.3e} cos {cs:.5f}")
    assert err < FREE_TOL and cs > FREE_COS
