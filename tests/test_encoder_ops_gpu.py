"""The small kernels of the text / vision towers (csrc/clip.hip, csrc/vit.hip, the one-wave-per-row LayerNorm of csrc/norm.hip)
on their own, per element: the towers' model-level gates (rel-L2 1.5e-2 on synthetic weights) cannot see an error confined to a
tail chunk, a last token or one activation value.

Every operand lives between guard bands (tests/bounds.py) and check_guards() follows every launch.  References are fp64 from
the values the kernel reads; bounds are a priori (the docstrings say what each term counts), never fitted.

sd_op_clip_embed CLAMPS a token id outside [0, vocab) to the nearest row, as clip_embed_kernel does; it is the Python wrapper
(sonicdiffusionbayeslab_amd/clip.py) that refuses such ids.  test_clip_embed_clamps_ids_outside_the_vocabulary pins the clamp.

The 128-token text attention at head dim 64 asks for 129 KiB of dynamic LDS, which no product path requests: it launches on the
MI355X (160 KiB per workgroup), so the launcher's "1..128 tokens" stands and the refusal test sits at 129."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from sonicdiffusionbayeslab_amd import _lib
from tests.bounds import (ATOL_TINY, GELU_POLY, U32, assert_elementwise, assert_flip_budget, attention_elementwise, check_guards,
                          forget_guards, guarded, guarded_input, ln_restatements, norm_ref_bound, ulp_bf16)

SD_ACT_QUICK_GELU, SD_ACT_GELU = 0, 1            # include/sd_hip.h


def stream():
    return _lib.current_stream()


def r16(t):
    return t.to(torch.bfloat16).float()


def bits(t):
    """bf16 / fp32 values as integers: comparisons that must hold bit for bit (and see NaN payloads)."""
    t = t.detach().cpu().contiguous()
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


@pytest.fixture(autouse=True)
def _forget():
    yield
    torch.cuda.synchronize()
    forget_guards()


# ---- layernorm_kernel<false>: every width but 320 / 640 / 1280 ----------------------------------------------------------

LN_CASES = [
    (1, 8, 1e-5, False),         # one chunk, one live wave of four
    (5, 64, 1e-5, False),        # rows not a multiple of 4
    (77, 520, 1e-5, False),      # 65 chunks: exactly one lane owns a second chunk
    (154, 768, 1e-5, False),     # lanes 0..31 own two chunks, the rest one
    (257, 1024, 1e-5, False),
    (6, 1536, 1e-5, False),      # the maximum: three chunks per lane
    (154, 768, 1e-12, False),    # BERT's eps
    (154, 768, 1e-5, True),      # one channel at 60x the others' scale in every row, as real checkpoints have
]


def _ln_case(rows, C, outlier):
    g = torch.Generator().manual_seed(rows * 10000 + C + (1 if outlier else 0))
    x = torch.randn(rows, C, generator=g) * 3 + 1
    if outlier:
        x[:, 301] = x[:, 301] * 60
    gamma, beta = torch.randn(C, generator=g), torch.randn(C, generator=g)
    return r16(x), gamma, beta


@pytest.mark.parametrize("rows,C,eps,outlier", LN_CASES)
def test_layernorm_generic_kernel(sdlib, rows, C, eps, outlier):
    """Per element (norm_ref_bound) and by count (assert_flip_budget against the two-pass fp32 restatements, budget
    4 F_ref + 8), as tests/test_ops_gpu.py::test_layernorm.  Measured flips / F_ref / numel, in LN_CASES' order:
    0 / 0 / 8, 0 / 0 / 320, 2 / 9 / 40040, 4 / 8 / 118272, 7 / 28 / 263168, 0 / 1 / 9216, 7 / 13 / 118272 (eps 1e-12),
    2 / 10 / 118272 (outlier channel); worst err / bound 0.43 .. 0.50 (the output rounding)."""
    x, gamma, beta = _ln_case(rows, C, outlier)
    out = guarded((rows, C), torch.bfloat16, label="y")
    _lib.check(sdlib.sd_op_layernorm(stream(), guarded_input(x, torch.bfloat16, label="x").data_ptr(),
                                     guarded_input(gamma, label="gamma").data_ptr(), guarded_input(beta, label="beta").data_ptr(),
                                     out.data_ptr(), rows, C, eps), "sd_op_layernorm")
    torch.cuda.synchronize()
    check_guards()
    what = f"layernorm {rows}x{C} eps {eps:g}" + (" outlier channel" if outlier else "")
    n64, nb = norm_ref_bound(x, gamma, beta, C, eps, False)
    assert_elementwise(out, n64, nb, what, ("row", "c"))
    assert_flip_budget(out, n64, ln_restatements(x, gamma, beta, eps), "bf16", what, acc_bound=nb - ulp_bf16(n64))


def test_layernorm_refusals_launch_nothing(sdlib):
    x = guarded_input(torch.ones(4, 1544), torch.bfloat16, label="x")
    gamma, beta = guarded_input(torch.ones(1544), label="gamma"), guarded_input(torch.zeros(1544), label="beta")
    out = guarded((4, 1544), torch.bfloat16, label="y")
    for rows, C, word in ((4, 1544, "C=1544"), (4, 12, "C=12"), (0, 768, "no rows")):
        with pytest.raises(_lib.SdHipError, match=word):
            _lib.check(sdlib.sd_op_layernorm(stream(), x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), out.data_ptr(), rows, C, 1e-5))
    torch.cuda.synchronize()
    assert torch.isnan(out.float()).all()                        # nothing ran: the output still holds its fill
    check_guards()


# ---- clip_attn_kernel ------------------------------------------------------------------------------------------------

CLIP_ATTN_SHAPES = [(1, 1, 64), (3, 12, 64), (2, 16, 64), (2, 4, 16)]      # (B, heads, D)


def _clip_attention(sdlib, qkv, B, L, H, heads, label):
    out = guarded((B * L, H), torch.bfloat16, label="out")
    _lib.check(sdlib.sd_op_clip_attention(stream(), guarded_input(qkv, label="qkv").data_ptr(), out.data_ptr(), B, L, H, heads), label)
    torch.cuda.synchronize()
    check_guards()
    return out.cpu()


@pytest.mark.parametrize("L", [1, 2, 63, 64, 65, 77, 127, 128])
def test_clip_attention_per_element(sdlib, L):
    """attention_ref_bound with the causal mask, every (B, heads, D) of CLIP_ATTN_SHAPES.  L = 64 / 65 is where the block grows
    from one wave to two; L = 128 at D = 64 takes 129 KiB of dynamic LDS.  Measured worst err / bound over the shapes, per L:
    0 (one key: the output is v), 0.322, 0.324, 0.326, 0.327, 0.321, 0.326, 0.322."""
    for B, heads, D in CLIP_ATTN_SHAPES:
        H = heads * D
        g = torch.Generator().manual_seed(L * 1000 + B * 100 + heads)
        qkv = (torch.randn(B * L, 3 * H, generator=g) * 1.5).to(torch.bfloat16)
        out = _clip_attention(sdlib, qkv, B, L, H, heads, f"sd_op_clip_attention L={L} B={B} heads={heads} D={D}")
        q, k, v = (qkv[:, i * H:(i + 1) * H].float().view(B, L, H) for i in range(3))
        attention_elementwise(out.float().view(B, L, H), q, k, v, heads, D, f"clip attention L={L} B={B} heads={heads} d{D}",
                              causal=True)


@pytest.mark.parametrize("L", [65, 77, 128])
def test_clip_attention_rows_do_not_see_later_tokens(sdlib, L):
    """Causality on its own: with the q, k and v rows of every token after p turned into NaN, output rows 0..p keep their bits."""
    for B, heads, D in ((2, 16, 64), (2, 4, 16)):
        H = heads * D
        g = torch.Generator().manual_seed(L * 1000 + heads)
        qkv = (torch.randn(B * L, 3 * H, generator=g) * 1.5).to(torch.bfloat16)
        first = _clip_attention(sdlib, qkv, B, L, H, heads, "sd_op_clip_attention").view(B, L, H)
        assert torch.isfinite(first.float()).all()
        for p in (0, 40, L - 2):
            poisoned = qkv.clone().view(B, L, 3 * H)
            poisoned[:, p + 1:] = float("nan")
            again = _clip_attention(sdlib, poisoned.view(B * L, 3 * H), B, L, H, heads, "sd_op_clip_attention").view(B, L, H)
            assert torch.equal(bits(again[:, :p + 1]), bits(first[:, :p + 1])), \
                f"L={L} heads={heads} d{D}: rows 0..{p} change when the tokens after {p} do"
            assert torch.isnan(again[:, p + 1:].float()).all()   # (and the poisoned queries really ran)


def test_clip_attention_refusals_launch_nothing(sdlib):
    H = 64
    qkv = guarded_input(torch.zeros(129, 3 * H, dtype=torch.bfloat16), label="qkv")
    out = guarded((129, H), torch.bfloat16, label="out")

    def call(B, L, H_, heads, q=None, o=None):
        return sdlib.sd_op_clip_attention(stream(), q or qkv.data_ptr(), o or out.data_ptr(), B, L, H_, heads)

    for args, word in (((1, 0, H, 1), "0 tokens"), ((1, 129, H, 1), "129 tokens"), ((1, 8, H, 2), "head dim 32"),
                       ((65536, 1, H, 1), "B=65536"), ((0, 8, H, 1), "B=0")):
        with pytest.raises(_lib.SdHipError, match=word):
            _lib.check(call(*args))
    for q, o in ((qkv.data_ptr() + 1, None), (None, out.data_ptr() + 2)):
        with pytest.raises(_lib.SdHipError, match="aligned"):
            _lib.check(call(1, 8, H, 1, q, o))
    torch.cuda.synchronize()
    assert torch.isnan(out.float()).all()                        # nothing ran: the output still holds its fill
    check_guards()


# ---- clip_embed_kernel, vit_embed_kernel -----------------------------------------------------------------------------

def _clip_embed(sdlib, ids, tok, pos, B, L, H, vocab):
    out = guarded((B * L, H), torch.bfloat16, label="out")
    _lib.check(sdlib.sd_op_clip_embed(stream(), guarded_input(ids, label="ids").data_ptr(), guarded_input(tok, label="tok").data_ptr(),
                                      guarded_input(pos, label="pos").data_ptr(), out.data_ptr(), B * L, L, H, vocab), "sd_op_clip_embed")
    torch.cuda.synchronize()
    check_guards()
    return out.cpu()


def _embed_tables(g, vocab, L, H):
    return ((torch.randn(vocab, H, generator=g) * 2).to(torch.bfloat16), (torch.randn(L, H, generator=g) * 2).to(torch.bfloat16))


@pytest.mark.parametrize("B,L,H,vocab", [(1, 1, 2, 3), (3, 16, 64, 50), (2, 77, 768, 1000),
                                         (1, 77, 258, 7)])        # 129 channel pairs for 128 threads
def test_clip_embed_is_the_rounded_fp32_sum(sdlib, B, L, H, vocab):
    g = torch.Generator().manual_seed(B * 100000 + L * 1000 + H)
    tok, pos = _embed_tables(g, vocab, L, H)
    ids = torch.randint(0, vocab, (B * L,), generator=g, dtype=torch.int32)
    ids[-1] = vocab - 1
    if B * L >= 4:
        ids[0], ids[1], ids[2] = 0, vocab - 1, ids[3]            # both ends of the table, and a repeat
    out = _clip_embed(sdlib, ids, tok, pos, B, L, H, vocab)
    want = (tok[ids.long()].float() + pos.float().repeat(B, 1)).bfloat16()
    assert torch.equal(bits(out), bits(want)), f"{int((bits(out) != bits(want)).sum())} of {out.numel()} elements differ"


def test_clip_embed_clamps_ids_outside_the_vocabulary(sdlib):
    B, L, H, vocab = 2, 5, 66, 11
    g = torch.Generator().manual_seed(5)
    tok, pos = _embed_tables(g, vocab, L, H)
    ids = torch.tensor([-1, vocab, 3, -2 ** 31, 2 ** 31 - 1, vocab - 1, 0, -1, vocab, 4], dtype=torch.int32)
    out = _clip_embed(sdlib, ids, tok, pos, B, L, H, vocab)
    want = (tok[ids.long().clamp(0, vocab - 1)].float() + pos.float().repeat(B, 1)).bfloat16()
    assert torch.equal(bits(out), bits(want))


@pytest.mark.parametrize("B,Np,H", [(2, 4, 64), (1, 49, 768), (3, 256, 1024)])
def test_vit_embed_is_the_rounded_fp32_sum(sdlib, B, Np, H):
    g = torch.Generator().manual_seed(B * 100000 + Np * 1000 + H)
    prow = (torch.randn(B * Np, H, generator=g) * 2).to(torch.bfloat16)
    pos = (torch.randn(Np + 1, H, generator=g) * 2).to(torch.bfloat16)
    cls = torch.randn(H, generator=g)                            # fp32: not bf16 values
    assert not torch.equal(cls, r16(cls))
    out = guarded((B * (Np + 1), H), torch.bfloat16, label="out")
    _lib.check(sdlib.sd_op_vit_embed(stream(), guarded_input(prow, label="patch rows").data_ptr(), guarded_input(cls, label="cls").data_ptr(),
                                     guarded_input(pos, label="pos").data_ptr(), out.data_ptr(), B, Np, H), "sd_op_vit_embed")
    torch.cuda.synchronize()
    check_guards()
    got = out.cpu().view(B, Np + 1, H)
    want = torch.empty(B, Np + 1, H, dtype=torch.bfloat16)
    want[:, 0] = (cls + pos[0].float()).bfloat16()
    want[:, 1:] = (prow.float().view(B, Np, H) + pos[1:].float()).bfloat16()
    assert torch.equal(bits(got), bits(want)), f"{int((bits(got) != bits(want)).sum())} of {got.numel()} elements differ"
    for b in range(1, B):
        assert torch.equal(bits(got[b, 0]), bits(got[0, 0]))


# ---- quick_gelu_kernel, gelu_erf_kernel ------------------------------------------------------------------------------

def bf16_finite_zero_or_normal():
    """Every bf16 bit pattern that is finite and zero or normal: 65536 - 256 inf / NaN - 254 subnormals = 65026 values."""
    code = torch.arange(65536, dtype=torch.int32)
    exp, man = (code >> 7) & 0xFF, code & 0x7F
    keep = (exp != 0xFF) & ((exp != 0) | (man == 0))
    code = code[keep]
    x = (code - ((code >= 32768).int() << 16)).to(torch.int16).view(torch.bfloat16)
    assert x.numel() == 65026
    return x


TAIL, TAIL_BITS = 64, 0x4242                                     # elements past n inside the same buffer, and what they hold


def _activate(sdlib, x, kind):
    """In place on the first x.numel() elements of a guarded buffer that is TAIL elements longer."""
    n = x.numel()
    buf = torch.cat([x.view(torch.int16), torch.full((TAIL,), TAIL_BITS, dtype=torch.int16)]).view(torch.bfloat16)
    d = guarded_input(buf, label="x")
    _lib.check(sdlib.sd_op_activation(stream(), d.data_ptr(), n, kind), "sd_op_activation")
    torch.cuda.synchronize()
    check_guards()
    got = d.cpu()
    assert (bits(got[n:]) == TAIL_BITS).all(), "the kernel wrote past n"
    return got[:n]


@pytest.mark.parametrize("extra", [0, 2])
@pytest.mark.parametrize("kind", [SD_ACT_QUICK_GELU, SD_ACT_GELU])
def test_activation_over_every_bf16_input(sdlib, kind, extra):
    """Every finite zero-or-normal bf16 value (65026; with two more the last block's 256 pairs end elsewhere) against fp64:
    gelu       |err| <= ulp_bf16(ref) / 2 + GELU_POLY |x| + tiny      (the formula's documented error, then one rounding);
    quick_gelu |err| <= ulp_bf16(ref) / 2 + (4 + 2 * 1.702 |x|) u32 |ref| + tiny: one rounded product 1.702 x and its scaling to
               an exp2 argument (each moves e^{1.702 x} by 1.702 |x| u32), the fast exp2, the add and the divide.
    Measured worst err / bound: quick_gelu 0.9998 (what the correctly rounded fp64 value gives: the bound is the half ulp and
    1e-5 more), gelu 0.9959, at either length."""
    x = bf16_finite_zero_or_normal()
    if extra:
        x = torch.cat([x, torch.tensor([1.0, -1.0], dtype=torch.bfloat16)])
    got = _activate(sdlib, x, kind)
    xd = x.double()
    if kind == SD_ACT_GELU:
        ref = xd * 0.5 * torch.special.erfc(-xd / math.sqrt(2.0))
        bound = ulp_bf16(ref) / 2 + GELU_POLY * xd.abs() + ATOL_TINY
    else:
        ref = xd * torch.sigmoid(1.702 * xd)
        bound = ulp_bf16(ref) / 2 + (4 + 2 * 1.702 * xd.abs()) * U32 * ref.abs() + ATOL_TINY
    assert_elementwise(got, ref, bound, f"{'gelu' if kind else 'quick_gelu'} over {x.numel()} bf16 values", ("i",))


@pytest.mark.parametrize("kind", [SD_ACT_QUICK_GELU, SD_ACT_GELU])
def test_activation_of_nan_and_signed_zeros(sdlib, kind):
    x = torch.tensor([float("nan"), -0.0, 0.0, 1.0, -float("nan"), 0.0, -0.0, float("nan")], dtype=torch.bfloat16)
    got = _activate(sdlib, x, kind).float()
    nan = torch.isnan(x.float())
    assert torch.isnan(got[nan]).all() and torch.isfinite(got[~nan]).all()
    assert (got[x.float() == 0] == 0).all()
    assert got[3] > 0.8


def test_activation_refusals_launch_nothing(sdlib):
    x = guarded_input(torch.full((8,), 3.0), torch.bfloat16, label="x")
    for n, kind, word in ((8, 2, "kind 2"), (8, -1, "kind -1"), (7, SD_ACT_GELU, "n=7"), (0, SD_ACT_QUICK_GELU, "n=0")):
        with pytest.raises(_lib.SdHipError, match=word):
            _lib.check(sdlib.sd_op_activation(stream(), x.data_ptr(), n, kind))
    torch.cuda.synchronize()
    assert (x.float().cpu() == 3.0).all()
    check_guards()


# ---- pool_rows_kernel ------------------------------------------------------------------------------------------------

EOS = 2                                                           # below every other id: the argmax rule would pick another row


def _ids_row(kind, L, g):
    """One row of token ids (values 3 .. 999, none equal to EOS) for a pooling rule's case."""
    row = torch.randint(3, 1000, (L,), generator=g, dtype=torch.int32)
    if kind == "several eos":
        row[[L // 3, L // 2, L - 1]] = EOS
    elif kind == "eos first":
        row[0] = EOS
    elif kind == "eos last":
        row[L - 1] = EOS
    elif kind == "unique max":
        row[(2 * L) // 3] = 5000
    elif kind == "tied max":
        row[[L // 4, L // 2, L - 1]] = 5000
    elif kind == "all equal":
        row[:] = 7
    else:
        assert kind == "no eos"
    return row


def _pool(sdlib, src, ids, B, L, H, eos_id):
    dst = guarded((B, H), torch.bfloat16, label="dst")
    idp = guarded_input(ids, label="ids").data_ptr() if ids is not None else None
    _lib.check(sdlib.sd_op_pool_rows(stream(), guarded_input(src, label="src").data_ptr(), idp, B, L, H, eos_id, dst.data_ptr()),
               "sd_op_pool_rows")
    torch.cuda.synchronize()
    check_guards()
    return dst.cpu()


@pytest.mark.parametrize("B,L,H", [(1, 1, 2), (5, 77, 768), (3, 16, 1000)])
def test_pool_rows_copies_the_row_transformers_pools(sdlib, B, L, H):
    """dst is a bit-exact copy of the row at torch.argmax(ids) (eos_id < 0) or at the first eos_id ((ids == eos).int().argmax:
    0 without one), or of row 0 without ids.  Every sample takes every case in turn."""
    g = torch.Generator().manual_seed(B * 100000 + L * 1000 + H)
    src = (torch.randn(B * L, H, generator=g) * 2).to(torch.bfloat16)
    rows = src.view(B, L, H)
    for eos_id, kinds in ((EOS, ("several eos", "eos first", "eos last", "no eos")), (-1, ("unique max", "tied max", "all equal"))):
        for shift in range(len(kinds)):
            ids = torch.stack([_ids_row(kinds[(b + shift) % len(kinds)], L, g) for b in range(B)])
            pos = (ids == eos_id).int().argmax(-1) if eos_id >= 0 else torch.argmax(ids, -1)
            got = _pool(sdlib, src, ids.reshape(-1), B, L, H, eos_id)
            want = rows[torch.arange(B), pos.long()]
            assert torch.equal(bits(got), bits(want)), f"eos_id {eos_id}, cases from {kinds[shift]!r}: expected positions {pos.tolist()}"
    got = _pool(sdlib, src, None, B, L, H, EOS)
    assert torch.equal(bits(got), bits(rows[:, 0]))


# ---- sd_clip_score ---------------------------------------------------------------------------------------------------

def _score(sdlib, x, y, want_raw=True, want_score=True):
    B, P = x.shape
    raw = guarded((B,), torch.float32, label="raw") if want_raw else None
    score = guarded((B,), torch.float32, label="score") if want_score else None
    _lib.check(sdlib.sd_clip_score(stream(), guarded_input(x, label="image embeds").data_ptr(), guarded_input(y, label="text embeds").data_ptr(),
                                   B, P, _lib.ptr(raw), _lib.ptr(score)), "sd_clip_score")
    torch.cuda.synchronize()
    check_guards()
    return (raw.cpu() if want_raw else None), (score.cpu() if want_score else None)


@pytest.mark.parametrize("P", [1, 5, 64, 512, 768, 1000])
@pytest.mark.parametrize("B", [1, 7])
def test_clip_score_per_pair(sdlib, B, P):
    """raw = 100 cos against fp64, |err| <= 100 (P + 16) u32 (sum |x_i y_i| / (|x| |y|) + |cos|) + tiny: three fp32 sums of P
    terms in any order, two square roots, a product, a divide and the scaling (the counting of
    tests/test_image_reward_gpu.py::test_reward_head_per_element); score = max(raw, 0) exactly; the one-output forms give the
    two-output call's bits.  Measured worst err / bound: 7.9e-2 (B = 7, P = 5), 3.7e-2 (B = 1, P = 5), <= 6.6e-3 from P = 64 on,
    0 at P = 1."""
    g = torch.Generator().manual_seed(B * 10000 + P)
    x = torch.randn(B, P, generator=g)
    y = torch.randn(B, P, generator=g)
    y[::2] = y[::2] + 0.5 * x[::2]                               # (every other pair correlated, as a matching caption is)
    raw, score = _score(sdlib, x, y)
    xd, yd = x.double(), y.double()
    nn = xd.norm(dim=-1) * yd.norm(dim=-1)
    cos = (xd * yd).sum(-1) / nn
    bound = 100 * (P + 16) * U32 * ((xd * yd).abs().sum(-1) / nn + cos.abs()) + ATOL_TINY
    assert_elementwise(raw, 100 * cos, bound, f"clip score B={B} P={P}", ("b",))
    assert torch.equal(score, raw.clamp(min=0.0))
    raw_only, _ = _score(sdlib, x, y, want_score=False)
    _, score_only = _score(sdlib, x, y, want_raw=False)
    assert torch.equal(bits(raw_only), bits(raw)) and torch.equal(bits(score_only), bits(score))


def test_clip_score_of_an_opposed_pair_and_of_a_zero_embedding(sdlib):
    g = torch.Generator().manual_seed(3)
    P = 768
    x = torch.randn(3, P, generator=g)
    y = torch.randn(3, P, generator=g)
    y[0] = -x[0] + 0.1 * y[0]                                    # cos ~ -0.995
    x[1] = 0.0                                                   # a zero image embedding
    raw, score = _score(sdlib, x, y)
    assert raw[0] < -99.0 and score[0] == 0.0                    # clamped to zero exactly, not to something small
    assert bits(raw)[1] & 0x7FFFFFFF == 0 and bits(score)[1] & 0x7FFFFFFF == 0
    assert torch.isfinite(raw).all() and torch.isfinite(score).all()


def test_clip_score_without_an_output_is_refused(sdlib):
    x = guarded_input(torch.ones(2, 8), label="image embeds")
    with pytest.raises(_lib.SdHipError, match="clip_score"):
        _lib.check(sdlib.sd_clip_score(stream(), x.data_ptr(), x.data_ptr(), 2, 8, None, None))
    torch.cuda.synchronize()
    check_guards()
