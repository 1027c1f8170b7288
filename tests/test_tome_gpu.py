"""Token Merging on the GPU: the four kernels of csrc/tome.hip against tests/tome_oracle.py per element, the UNet forward with
the library's own matchings fed to the oracle, and the pipelines.  The kernels at the level that merges at 512 px (64x64 tokens,
C = 320) and at the admitted limits; the self-attention at the row counts merging produces (N - int(N ratio): 717, 2663, ...);
the UNet at ratios 0.25 / 0.3 / 0.75 and on the head-major K / V path (profiles/tome_notes.md has the measured figures).

Tolerances.  ``tome_match`` multiplies the RAW bf16 rows on the MFMA and scales the fp32 accumulator by the two fp32 inverse
norms afterwards (csrc/tome.hip, "Precision of the match"): no unit row is rounded to bf16, so against the exact cosine of
the same bf16 rows the error is the fp32 accumulation's (C 2^-24 on the unit scale), the same for each of the two sums of
squares and a few ulp for sqrt, divide and the two multiplies: eps = 4 C 2^-24 (3e-4 at C = 1280; the 2^-8 of bf16 unit rows
does not apply).  Merge: one bf16 ulp of the result + 2^-24 (1 + count) mag; unmerge: one ulp + 2 * 2^-24 mag."""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from sonicdiffusionbayeslab_amd import _lib
from tests import tome_oracle as to
from tests.bounds import (ATOL_TINY, assert_elementwise, attention_elementwise, check_guards, forget_guards, guarded, guarded_input,
                          ulp_bf16)
from tests.util import rel_l2, synth_inputs

UNET_TOL = 2e-2                     # tests/test_unet_gpu.py
FREE_TOL = 6e-2                     # tests/test_pipeline_gpu.py
U32 = 2.0 ** -24

#        B  h   w   C
CASES = {"a": (2, 8, 6, 320),        # 36 src / 12 dst: ragged against every tile
         "b": (3, 32, 32, 640),      # 768 / 256: several src and dst tiles, the argmax crosses tiles
         "c": (1, 24, 40, 1280),     # non-square
         "d": (1, 64, 64, 320),      # 3072 / 1024: level 0 at 512 px, the level that merges
         "e": (1, 128, 128, 320),    # 12288 / 4096: the admitted maximum (12 items per select thread); its own test only
         "f": (2, 2, 2, 64),         # 3 / 1: the admitted minimum, one K chunk
         "g": (1, 6, 4, 1536)}       # the widest row: all three row chunks of merge full, 24 K chunks in the match
LOOPED = [c for c in CASES if c != "e"]          # what the tests below iterate ("e": test_the_admitted_maximum alone)
ATTN_TOL = 1e-2                     # tests/test_ops_gpu.py::test_attention: P rounded to bf16 before PV
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


def r16(t):
    return t.to(torch.bfloat16).float()


def r_values(h, w):
    n = h * w
    return sorted({1, int(n * 0.3), int(n * 0.35), int(n * 0.5), n - n // 4})


def make_choice(h, w, kind):
    cells = (h // 2) * (w // 2)
    if kind == "zero":
        return torch.zeros(cells, dtype=torch.uint8)
    return torch.randint(4, (cells,), generator=torch.Generator().manual_seed(h * 131 + w), dtype=torch.uint8)


def tokens(case, kind):
    """[B, N, C] fp32 values on the bf16 grid.  gauss: the best dst is far above a random one; smooth: an image-like field whose
    neighbours are nearly parallel (many near-ties); exact: four non-zeros of +-2^k per row at a small pool of channels, so norms,
    unit entries and scores are exact and exact ties abound, with one zero row and duplicated rows."""
    B, h, w, C = CASES[case]
    g = torch.Generator().manual_seed(sum(map(ord, case + kind)) + 17 * C)
    if kind == "gauss":
        return r16(torch.randn(B, h * w, C, generator=g))
    if kind == "smooth":
        yy, xx = torch.meshgrid(torch.arange(h, dtype=torch.float32), torch.arange(w, dtype=torch.float32), indexing="ij")
        f = torch.rand(3, C, generator=g) * 0.5
        ph = torch.rand(B, 1, 1, C, generator=g) * 6.28
        field = torch.sin(yy[None, :, :, None] * f[0] + xx[None, :, :, None] * f[1] + ph) + 0.5 * torch.cos(xx[None, :, :, None] * f[2])
        return r16(field.reshape(B, h * w, C) + 0.02 * torch.randn(B, h * w, C, generator=g))
    assert kind == "exact"
    N = h * w
    pool = torch.linspace(0, C - 1, 12).long()                      # 12 channels spread over every K chunk
    x = torch.zeros(B, N, C)
    for b in range(B):
        for t in range(N):
            pos = pool[torch.randperm(12, generator=g)[:4]]
            sign = torch.randint(2, (4,), generator=g).float() * 2 - 1
            x[b, t, pos] = sign * 2.0 ** int(torch.randint(-3, 4, (1,), generator=g))
        x[b, N // 3] = 0.0                                           # one zero row
        if N > 5:
            x[b, 5] = x[b, 1]
        x[b, N - 2] = x[b, 1]; x[b, N // 2] = x[b, 2]                # duplicated rows (2x2 tokens: rows 1 and 2 are one row, zero)
    return x


def gpu_match(sdlib, x, choice, h, w):
    B, N, C = x.shape
    num_src = N - N // 4
    nm = guarded((B, num_src), torch.float32, label="node_max")
    ni = guarded((B, num_src), torch.int32, fill=-1, label="node_idx")
    tok = guarded((1, N), torch.int32, fill=-1, label="tok")
    _lib.check(sdlib.sd_op_tome_match(stream(), P(guarded_input(x, torch.bfloat16)), P(guarded_input(choice.reshape(1, -1))), B, h, w, C,
                                      P(nm), P(ni), P(tok)))
    torch.cuda.synchronize()
    return nm.cpu(), ni.cpu(), tok.cpu().reshape(-1)


def gpu_select(sdlib, node_max, node_idx, r):
    B, num_src = node_max.shape
    # (an empty list -- r = 0 or r = num_src -- is a NULL pointer)
    kept = guarded((B, num_src - r), torch.int32, fill=-1, label="kept") if num_src - r else None
    merged = guarded((B, r), torch.int32, fill=-1, label="merged") if r else None
    dst = guarded((B, r), torch.int32, fill=-1, label="dst_idx") if r else None
    ptr = lambda t: None if t is None else P(t)
    _lib.check(sdlib.sd_op_tome_select(stream(), P(guarded_input(node_max)), P(guarded_input(node_idx.to(torch.int32))), B, num_src, r,
                                       ptr(kept), ptr(merged), ptr(dst)))
    torch.cuda.synchronize()
    z = torch.zeros(B, 0, dtype=torch.int32)
    return tuple(z if t is None else t.cpu() for t in (kept, merged, dst))


# ------------------------------------------------------------------------------------------------------------- match
@pytest.mark.parametrize("kind", ["gauss", "smooth"])
@pytest.mark.parametrize("choice_kind", ["zero", "random"])
@pytest.mark.parametrize("case", LOOPED)
def test_match_tolerance(sdlib, case, choice_kind, kind):
    check_match(sdlib, case, choice_kind, kind)


def check_match(sdlib, case, choice_kind, kind):
    B, h, w, C = CASES[case]
    x, choice = tokens(case, kind), make_choice(h, w, choice_kind)
    eps = 4 * C * U32                                       # csrc/tome.hip: raw products, scaled afterwards
    nm, ni, tok = gpu_match(sdlib, x, choice, h, w)
    check_guards()
    src_tok, dst_tok = to.partition(choice, h, w)
    assert torch.equal(tok.long(), torch.cat([src_tok, dst_tok]))
    s = to.scores(x, src_tok, dst_tok)                      # fp64, from the same bf16 values
    assert ni.min() >= 0 and ni.max() < dst_tok.numel() and torch.isfinite(nm).all()
    chosen = torch.gather(s, 2, ni.long().unsqueeze(-1)).squeeze(-1)
    best = s.max(-1).values
    gap, err = float((best - chosen).max()), float((nm.double() - chosen).abs().max())
    # (s.argmax: some maximum; it differs from the first one only at an exact tie, which these inputs do not have)
    print(f"[tome match] {case} {kind} {choice_kind}: eps {eps:.2e}, worst (oracle max - oracle score of the chosen dst) {gap:.2e}, "
          f"worst |node_max - oracle score of the chosen dst| {err:.2e}, wrong indices {int((ni.long() != s.argmax(-1)).sum())}")
    assert (chosen >= best - 2 * eps).all()                 # no row excluded
    assert ((nm.double() - chosen).abs() <= eps).all()
    return x, choice, nm, ni, tok


@pytest.mark.parametrize("choice_kind", ["zero", "random"])
@pytest.mark.parametrize("case", LOOPED)
def test_match_and_select_exact(sdlib, case, choice_kind):
    """Exact inputs: node_idx, the merged set and dst_idx equal the oracle's element for element, ties included."""
    B, h, w, C = CASES[case]
    x, choice = tokens(case, "exact"), make_choice(h, w, choice_kind)
    nm, ni, tok = gpu_match(sdlib, x, choice, h, w)
    ref = to.match(x, choice, h, w, 0)
    assert not torch.isnan(nm).any()
    assert torch.equal(nm.double(), ref["node_max"])        # exact arithmetic on both sides
    assert torch.equal(ni.long(), ref["node_idx"])
    ties = int((to.scores(x, ref["src_tok"], ref["dst_tok"]) == ref["node_max"].unsqueeze(-1)).sum(-1).gt(1).sum())
    assert ties > 0 or ref["dst_tok"].numel() == 1            # the lowest-dst rule was exercised (one dst: no rule to exercise)
    for r in r_values(h, w):
        kept, merged, dst = gpu_select(sdlib, nm, ni, r)
        want_kept, want_merged = to.select(ref["node_max"], r)
        assert torch.equal(merged.long(), want_merged), r
        assert torch.equal(kept.long(), want_kept), r
        assert torch.equal(dst.long(), torch.gather(ref["node_idx"], 1, want_merged)), r
    check_guards()


# ------------------------------------------------------------------------------------------------------------ select
@pytest.mark.parametrize("num_src", [36, 768, 1000, 12288])
def test_select_arbitrary_scores(sdlib, num_src):
    g = torch.Generator().manual_seed(num_src)
    B = 3
    s = torch.randn(B, num_src, generator=g)
    s[0] = (s[0] * 4).round() / 4                           # many equal values
    s[1, ::7] = 0.0; s[1, 3::7] = -0.0                      # +-0 are one value
    s[1, 1::7] = 1e-42; s[1, 2::7] = -1e-42; s[1, 5::7] = 2e-45     # denormals order like any other value
    s[2, : num_src // 2] = 0.5                              # a long run of ties across the cut
    idx = torch.randint(0, max(num_src // 3, 1), (B, num_src), generator=g, dtype=torch.int32)
    for r in sorted({0, 1, num_src // 3, num_src // 2, num_src - 1, num_src}):
        kept, merged, dst = gpu_select(sdlib, s, idx, r)
        assert merged.shape == (B, r) and kept.shape == (B, num_src - r)
        for b in range(B):
            m, k = merged[b].long(), kept[b].long()
            assert torch.equal(torch.cat([m, k]).sort().values, torch.arange(num_src))          # disjoint, union = all src
            assert (m[1:] > m[:-1]).all() and (k[1:] > k[:-1]).all()                            # ascending
            if 0 < r < num_src:
                cut = s[b, m].min()
                assert cut >= s[b, k].max()
                at_cut_m, at_cut_k = m[s[b, m] == cut], k[s[b, k] == cut]
                assert at_cut_k.numel() == 0 or at_cut_m.max() < at_cut_k.min()                 # the index tiebreak at the cut
            assert torch.equal(dst[b], idx[b, m])
        want_kept, want_merged = to.select(s, r)
        assert torch.equal(merged.long(), want_merged) and torch.equal(kept.long(), want_kept)
    check_guards()


# ---------------------------------------------------------------------------------------------------- merge / unmerge
def gpu_merge(sdlib, x, tok, kept, merged, dst, h, w, r, ldo=None):
    """``ldo``: the row pitch of the output (default C); the gap columns hold the guards' sentinel (tests/bounds.py)."""
    B, N, C = x.shape
    out = guarded((B * (N - r), C), torch.bfloat16, ld=ldo, label="merged rows")
    i32 = lambda t: P(guarded_input(t.to(torch.int32).reshape(1, -1))) if t.numel() else None
    _lib.check(sdlib.sd_op_tome_merge(stream(), P(guarded_input(x.reshape(B * N, C), torch.bfloat16)), i32(tok), i32(kept), i32(merged),
                                      i32(dst), P(out), ldo or C, B, h, w, C, r))
    torch.cuda.synchronize()
    return out.float().cpu().reshape(B, N - r, C)


def gpu_unmerge(sdlib, y, res, tok, kept, merged, dst, h, w, r, ldy=None):
    """``res`` None: no residual (a NULL pointer); ``ldy``: the row pitch of y (default C), its gap columns NaN."""
    B, C = y.shape[0], y.shape[2]
    N = h * w
    out = guarded((B * N, C), torch.bfloat16, label="unmerged rows")
    i32 = lambda t: P(guarded_input(t.to(torch.int32).reshape(1, -1))) if t.numel() else None
    _lib.check(sdlib.sd_op_tome_unmerge(stream(), P(guarded_input(y.reshape(B * (N - r), C), torch.bfloat16, ld=ldy)), ldy or C,
                                        None if res is None else P(guarded_input(res.reshape(B * N, C), torch.bfloat16)), i32(tok),
                                        i32(kept), i32(merged), i32(dst), P(out), B, h, w, C, r))
    torch.cuda.synchronize()
    return out.float().cpu().reshape(B, N, C)


def check_merge_unmerge(sdlib, case, x, choice, kept, merged, dst, what):
    B, h, w, C = CASES[case]
    N, r = h * w, merged.shape[1]
    src_tok, dst_tok = to.partition(choice, h, w)
    tok = torch.cat([src_tok, dst_tok])
    args = (src_tok, dst_tok, kept, merged, dst)
    got = gpu_merge(sdlib, x, tok, kept, merged, dst, h, w, r)
    ref = to.merge(x.double(), *args)
    cnt = to.member_counts(dst, dst_tok.numel()).double()                    # 1 + members
    count_row = torch.cat([torch.ones(B, N - r - dst_tok.numel(), dtype=torch.float64), cnt], 1).unsqueeze(-1)
    mag = to.merge(x.double().abs(), *args)                                  # the mean of the |terms|: (sum of |terms|) / count
    assert_elementwise(got, ref, ulp_bf16(ref) + U32 * (1 + count_row) * mag + ATOL_TINY, f"tome_merge {what}", ("b", "row", "c"))
    g = torch.Generator().manual_seed(r + 1)
    y, res = r16(torch.randn(B, N - r, C, generator=g)), r16(torch.randn(B, N, C, generator=g))
    gu = gpu_unmerge(sdlib, y, res, tok, kept, merged, dst, h, w, r)
    a = to.unmerge(y.double(), *args)
    ru = a + res.double()
    assert_elementwise(gu, ru, ulp_bf16(ru) + 2 * U32 * (a.abs() + res.double().abs()) + ATOL_TINY, f"tome_unmerge {what}", ("b", "token", "c"))
    check_guards()
    return got, gu


@pytest.mark.parametrize("choice_kind", ["zero", "random"])
@pytest.mark.parametrize("case", LOOPED)
def test_merge_unmerge_against_oracle(sdlib, case, choice_kind):
    B, h, w, C = CASES[case]
    x, choice = tokens(case, "smooth"), make_choice(h, w, choice_kind)
    for r in r_values(h, w):
        m = to.match(x, choice, h, w, r)
        check_merge_unmerge(sdlib, case, x, choice, m["kept"], m["merged"], m["dst_idx"], f"{case} r={r} {choice_kind}")


def test_merge_with_an_empty_dst_and_a_dst_of_more_than_64_members(sdlib):
    B, h, w, C = CASES["b"]
    x, choice = tokens("b", "gauss"), make_choice(h, w, "random")
    num_src, num_dst, r = 768, 256, 384
    g = torch.Generator().manual_seed(4)
    merged = torch.stack([torch.randperm(num_src, generator=g)[:r].sort().values for _ in range(B)])
    kept = torch.stack([torch.tensor(sorted(set(range(num_src)) - set(m.tolist()))) for m in merged])
    dst = torch.randint(8, num_dst, (B, r), generator=g)          # dst 0..7 receive nothing at random ...
    dst[:, :100] = 5                                              # ... dst 5 receives 100 members, dst 7 none
    cnt = to.member_counts(dst, num_dst)
    assert (cnt[:, 5] == 101).all() and (cnt[:, 7] == 1).all()
    got, _ = check_merge_unmerge(sdlib, "b", x, choice, kept, merged, dst, "b crafted")
    _, dst_tok = to.partition(choice, h, w)
    assert torch.equal(got[:, num_src - r + 7], x[:, dst_tok[7]])                 # no members: the dst row itself


def test_kernels_are_deterministic(sdlib):
    B, h, w, C = CASES["b"]
    x, choice = tokens("b", "smooth"), make_choice(h, w, "random")
    r = int(h * w * 0.5)
    runs = []
    for _ in range(2):
        nm, ni, tok = gpu_match(sdlib, x, choice, h, w)
        kept, merged, dst = gpu_select(sdlib, nm, ni, r)
        y = gpu_merge(sdlib, x, tok, kept, merged, dst, h, w, r)
        u = gpu_unmerge(sdlib, y, x, tok, kept, merged, dst, h, w, r)
        runs.append((nm, ni, tok, kept, merged, dst, y, u))
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def test_the_admitted_maximum(sdlib):
    """128x128 tokens: 12288 src (12 scores per select thread, the most tome_select_kernel holds) against 4096 dst.  The match
    against the fp64 scores (about 400 MB: computed once, here only); then select, merge and unmerge on the KERNEL's node_max /
    node_idx at the r of ratio 0.5 -- the oracle's select of the same fp32 scores must give the same lists."""
    B, h, w, C = CASES["e"]
    x, choice, nm, ni, tok = check_match(sdlib, "e", "random", "gauss")
    r = int(h * w * 0.5)
    assert nm.shape == (1, 12288) and r == 8192
    kept, merged, dst = gpu_select(sdlib, nm, ni, r)
    want_kept, want_merged = to.select(nm, r)
    assert torch.equal(merged.long(), want_merged) and torch.equal(kept.long(), want_kept)
    assert torch.equal(dst.long(), torch.gather(ni.long(), 1, want_merged))
    check_merge_unmerge(sdlib, "e", x, choice, kept.long(), merged.long(), dst.long(), "e r=8192 on the kernel's own match")


@pytest.mark.parametrize("case", ["a", "g"])
def test_merge_and_unmerge_with_a_row_pitch_wider_than_the_row(sdlib, case):
    """ldo = C + 64 at the merge, ldy = C + 64 at the unmerge (the C ABI takes them; the plan passes C): the padding columns keep
    what was there (the guards' sentinel, check_guards) and the rows equal the contiguous call's bit for bit."""
    B, h, w, C = CASES[case]
    N = h * w
    x, choice = tokens(case, "smooth"), make_choice(h, w, "random")
    for r in (int(N * 0.35), N - N // 4):
        m = to.match(x, choice, h, w, r)
        idx = (m["kept"], m["merged"], m["dst_idx"])
        tok = torch.cat([m["src_tok"], m["dst_tok"]])
        flat = gpu_merge(sdlib, x, tok, *idx, h, w, r)
        wide = gpu_merge(sdlib, x, tok, *idx, h, w, r, ldo=C + 64)
        assert torch.isfinite(flat).all() and torch.equal(wide, flat), r
        g = torch.Generator().manual_seed(r + 2)
        y, res = r16(torch.randn(B, N - r, C, generator=g)), r16(torch.randn(B, N, C, generator=g))
        flat = gpu_unmerge(sdlib, y, res, tok, *idx, h, w, r)
        wide = gpu_unmerge(sdlib, y, res, tok, *idx, h, w, r, ldy=C + 64)
        assert torch.isfinite(flat).all() and torch.equal(wide, flat), r
        check_guards()


@pytest.mark.parametrize("case", ["a", "g"])
def test_unmerge_without_a_residual_is_the_copy_of_the_rows(sdlib, case):
    B, h, w, C = CASES[case]
    N = h * w
    x, choice = tokens(case, "smooth"), make_choice(h, w, "random")
    for r in (int(N * 0.35), N - N // 4):
        m = to.match(x, choice, h, w, r)
        args = (m["src_tok"], m["dst_tok"], m["kept"], m["merged"], m["dst_idx"])
        y = r16(torch.randn(B, N - r, C, generator=torch.Generator().manual_seed(r + 3)))
        got = gpu_unmerge(sdlib, y, None, torch.cat(args[:2]), *args[2:], h, w, r)
        assert torch.equal(got, to.unmerge(y, *args)), r
        check_guards()


def test_the_ops_refuse_what_sd_tome_check_refuses(sdlib):
    """Shapes and counts outside the admitted ones: a non-zero return before any launch, the offending value in sd_last_error,
    and the outputs (NaN / -1 between their guards) as they were."""
    def buffers(B, h, w, C, r, ld=None):
        N = h * w
        num_src = N - (h // 2) * (w // 2)
        rr = max(min(r, num_src), 1)
        z = lambda *s: P(guarded_input(torch.zeros(*s, dtype=torch.int32)))
        f = dict(nm=guarded((B, num_src), torch.float32, label="node_max"), ni=guarded((B, num_src), torch.int32, fill=-1, label="node_idx"),
                 tok=guarded((1, N), torch.int32, fill=-1, label="tok"), out=guarded((B * N, max(C, ld or C)), torch.bfloat16, label="rows"))
        return f, P(guarded_input(torch.zeros(B * N, C), torch.bfloat16)), P(guarded_input(torch.zeros(1, (h // 2) * (w // 2), dtype=torch.uint8))), \
            z(1, N), z(B, max(num_src - rr, 1)), z(B, rr), z(B, rr)

    def untouched(f):
        torch.cuda.synchronize()
        assert torch.isnan(f["nm"]).all() and torch.isnan(f["out"].float()).all()
        assert (f["ni"] == -1).all() and (f["tok"] == -1).all()
        check_guards()

    def refused(rc, *names):
        err = sdlib.sd_last_error()
        assert rc != 0 and all(n in err for n in names), (rc, err, names)

    # B  h    w    C     what sd_last_error names
    for B, h, w, C, name in ((1, 6, 5, 320, b"6x5"), (1, 130, 128, 64, b"130x128"), (1, 8, 6, 96, b"C=96"), (1, 8, 6, 1600, b"C=1600")):
        r = 4
        f, x, choice, tok, kept, merged, dst = buffers(B, h, w, C, r)
        refused(sdlib.sd_op_tome_match(stream(), x, choice, B, h, w, C, P(f["nm"]), P(f["ni"]), P(f["tok"])), name, b"tome_match")
        refused(sdlib.sd_op_tome_merge(stream(), x, tok, kept, merged, dst, P(f["out"]), C, B, h, w, C, r), name, b"tome_merge")
        refused(sdlib.sd_op_tome_unmerge(stream(), x, C, x, tok, kept, merged, dst, P(f["out"]), B, h, w, C, r), name, b"tome_unmerge")
        untouched(f)
    B, h, w, C = CASES["a"]
    num_src = 36
    f, x, choice, tok, kept, merged, dst = buffers(B, h, w, C, num_src + 1)
    refused(sdlib.sd_op_tome_merge(stream(), x, tok, kept, merged, dst, P(f["out"]), C, B, h, w, C, num_src + 1), b"r=37 of 36")
    refused(sdlib.sd_op_tome_unmerge(stream(), x, C, x, tok, kept, merged, dst, P(f["out"]), B, h, w, C, num_src + 1), b"r=37 of 36")
    refused(sdlib.sd_op_tome_select(stream(), x, tok, B, num_src, num_src + 1, kept, merged, dst), b"r=37 of 36")
    refused(sdlib.sd_op_tome_merge(stream(), x, tok, kept, merged, dst, P(f["out"]), C - 8, B, h, w, C, 4), b"ldo=312")
    refused(sdlib.sd_op_tome_unmerge(stream(), x, C - 8, x, tok, kept, merged, dst, P(f["out"]), B, h, w, C, 4), b"ldy=312")
    untouched(f)
    sel = [guarded((1, 12289), torch.int32, fill=-1, label=n) for n in ("kept", "merged", "dst_idx")]
    scores = P(guarded_input(torch.zeros(1, 12289)))
    refused(sdlib.sd_op_tome_select(stream(), scores, P(guarded_input(torch.zeros(1, 12289, dtype=torch.int32))), 1, 12289, 100,
                                    *(P(t) for t in sel)), b"12289")
    torch.cuda.synchronize()
    assert all((t == -1).all() for t in sel)
    check_guards()


# ------------------------------------------------------------------------------------------------------ UNet forward
# ------------------------------------------------------------------------------------- attention at merged row counts
# (d, heads, B, Nk, tokens of the level, ratio): the self-attention of a merging block runs on Nk = N - int(N ratio) rows per sample,
# whatever that number is.  d = 40: level 0 of SD 1.x at 64x64 / 32x32 / 16x16 latents; d = 80: its level 1 at 32x32 / 64x64
# latents; d = 64: SD 2.x, 5 heads on level 0 and 10 on level 1.  Kernels (csrc/attention.hip::sd_launch_attention), none of
# these key counts being a multiple of 64: d = 40 -> attn_dma_kernel<40> (run at 77 and 300 keys elsewhere), d = 80 ->
# attn_kernel<80> (never at an odd key count elsewhere), d = 64 -> attn_kernel<64>.  B = 2: the per-sample stride.
MERGED_ATTN = [(40, 8, 1, 717, 1024, 0.3), (40, 8, 1, 2663, 4096, 0.35), (40, 8, 1, 2868, 4096, 0.3), (40, 8, 2, 180, 256, 0.3),
               (80, 8, 2, 167, 256, 0.35), (80, 8, 2, 180, 256, 0.3), (80, 8, 2, 717, 1024, 0.3),
               (64, 5, 2, 167, 256, 0.35), (64, 10, 2, 167, 256, 0.35), (64, 5, 2, 717, 1024, 0.3), (64, 10, 2, 717, 1024, 0.3)]


@pytest.mark.parametrize("spike", [False, True], ids=["plain", "spike"])
@pytest.mark.parametrize("D,heads,B,Nk,N,ratio", MERGED_ATTN)
def test_attention_at_merged_row_counts(sdlib, D, heads, B, Nk, N, ratio, spike):
    """Inputs as tests/test_resolution_edges_gpu.py::test_attention_at_odd_level_token_counts draws them; ``spike``: key Nk - 3
    times 6 (its test_attention_moderate_key_spike_in_the_ragged_last_tile), so that the ragged last tile carries weight.  q, k
    and v interleaved in one buffer with row stride 3 C, as the merging plan passes its q|k|v GEMM's output."""
    assert Nk == N - int(N * ratio) == N - to.num_merged(N, ratio) and Nk % 64 != 0
    C = heads * D
    g = torch.Generator().manual_seed(Nk * 8 + D + heads + spike)
    q, k, v = (r16(torch.randn(B, Nk, C, generator=g)) for _ in range(3))
    if spike:
        k[:, Nk - 3] = r16(k[:, Nk - 3] * 6)
    qh, kh, vh = (t.view(B, Nk, heads, D).transpose(1, 2) for t in (q, k, v))
    ref = F.scaled_dot_product_attention(qh, kh, vh).transpose(1, 2).reshape(B, Nk, C)
    qkv = guarded_input(torch.cat([q, k, v], dim=-1).reshape(B * Nk, 3 * C), torch.bfloat16)
    out = guarded((B, Nk, C), torch.bfloat16)
    base = P(qkv)
    _lib.check(sdlib.sd_op_attention(stream(), base, 3 * C, base + 2 * C, 3 * C, base + 4 * C, 3 * C, P(out), C, B, heads, Nk, Nk, D,
                                     1.0 / math.sqrt(D)))
    torch.cuda.synchronize()
    err = rel_l2(out, ref)
    print(f"[tome attention] d={D} heads={heads} B={B} Nk={Nk} ({N} tokens at ratio {ratio}) spike={int(spike)}: rel-L2 {err:.3e}")
    assert torch.isfinite(out.float()).all() and err < ATTN_TOL
    attention_elementwise(out, q, k, v, heads, D, f"attention merged rows d{D} h{heads} B={B} Nk={Nk} spike={int(spike)}")
    check_guards()


def _env(name):
    from sonicdiffusionbayeslab_amd.unet import HipUNet2DConditionModel
    cfg, sd, ocfg, heads = to.unet_env(name)
    return cfg, sd, HipUNet2DConditionModel(cfg, sd), ocfg, heads


@pytest.fixture(scope="module")
def tome_unet():
    return _env("sd15")


@pytest.fixture(scope="module")
def tome_sd2_unet():
    return _env("sd2")


@pytest.fixture(scope="module")
def tome_two_level_unet():
    return _env("two_level")


_PLAIN = {}          # the oracle's plain forward per (config, size, batch): computed once, shared by the cases, never changed


def forward_with_tome_and_check(env, h, w, lb, ub, md, ratio=0.5, t=981.0, n_blocks=None, seed=29):
    """``n_blocks``: how many blocks merge (default: the four-level UNet's two down and three up blocks per merging level)."""
    from oracle.unet import unet_forward
    cfg, sd, net, ocfg, heads = env
    lat, ctx, sample, choice = to.unet_inputs(cfg, h, w, lb, ub, md, seed)
    floor = to.moved_floor(ratio)
    key = (id(net), h, w, lb, ub, seed, t)
    if key not in _PLAIN:
        with torch.no_grad():
            if heads is not None:
                from tests.sd2_oracle import sd2_unet_forward
                _PLAIN[key] = sd2_unet_forward(sd, ocfg, heads, sample, t, ctx)
            else:
                _PLAIN[key] = unet_forward(sd, ocfg, sample, t, ctx)
    plain = _PLAIN[key]
    net.set_deepcache(-1)
    net.set_tome(ratio, md)
    try:
        blocks = net.tome_blocks(h, w)
        assert len(blocks) == (5 * md if n_blocks is None else n_blocks), blocks
        assert [(b["h"], b["w"]) for b in blocks] == to.merging_grids(cfg, h, w, md)      # the order the oracle calls them in
        cells = [(b["h"] // 2) * (b["w"] // 2) for b in blocks]
        assert [b["choice_off"] for b in blocks] == [sum(cells[:i]) for i in range(len(cells))]
        assert choice.numel() == sum(cells)
        net.set_context(ctx.cuda(), h, w)
        net.set_tome_choice(choice.cuda(), h, w)
        eps = net.forward_latents(lat.cuda(), ub, t)
        torch.cuda.synchronize()
        given, choices = [], []
        for i, b in enumerate(blocks):
            n = b["h"] * b["w"]
            num_src, num_dst, r = n - n // 4, n // 4, b["r"]
            assert r == to.num_merged(n, ratio)
            m = net.tome_matching(i, ub, h, w)
            c = choice[b["choice_off"]:b["choice_off"] + num_dst]
            src_tok, dst_tok = to.partition(c, b["h"], b["w"])
            assert m["r"] == r and torch.equal(m["tok"].long(), torch.cat([src_tok, dst_tok]))
            bm = m["kept"].shape[0]
            assert bm == (lb if (i == 0 and ub == 2 * lb) else ub)        # the first block of a CFG pair matches once per latent
            assert m["kept"].shape == (bm, num_src - r) and m["merged"].shape == (bm, r) and m["dst_idx"].shape == (bm, r)
            for s in range(bm):          # ranges, uniqueness, ascending order
                both = torch.cat([m["kept"][s], m["merged"][s]]).long()
                assert torch.equal(both.sort().values, torch.arange(num_src))
                assert (m["kept"][s][1:] > m["kept"][s][:-1]).all() and (m["merged"][s][1:] > m["merged"][s][:-1]).all()
                assert m["dst_idx"][s].min() >= 0 and m["dst_idx"][s].max() < num_dst
            if ratio == 0.75:            # r = num_src: nothing is kept, every src slot is merged
                assert r == num_src and m["kept"].shape == (bm, 0)
                assert torch.equal(m["merged"].long(), torch.arange(num_src).expand(bm, num_src))
            rep = ub // bm
            given.append({k: m[k].repeat(rep, 1) for k in ("kept", "merged", "dst_idx")})
            choices.append(c)
        run = to.TomeRun((h, w), ratio, md, choices, given=given)
        ref = to.unet_forward(sd, ocfg, sample, t, ctx, run, heads_per_level=heads)
        assert len(run.used) == len(blocks)
        own = rel_l2(ref, plain)
        err, moved = rel_l2(eps, ref), rel_l2(eps, plain)
        print(f"[tome unet] {h}x{w} batch {lb}/{ub} max_downsample {md} ratio {ratio}: rel-L2 vs oracle with the library's matchings "
              f"{err:.3e}; vs the plain oracle {moved:.3f} (oracle's own with / without {own:.3f}, floor {floor:.2f})")
        assert own > floor
        assert torch.isfinite(eps).all() and err < UNET_TOL
        assert moved > floor
        return eps, blocks
    finally:
        net.set_tome(0.0)


def _cases(name):
    return [pytest.param(*c[1:], id=f"{c[1]}x{c[2]}-b{c[3]}_{c[4]}-r{c[6]}") for c in to.UNET_CASES if c[0] == name]


@pytest.mark.parametrize("h,w,lb,ub,md,ratio,n_blocks,seed,t", _cases("sd15"))
def test_unet_forward_with_tome_beyond_ratio_half(tome_unet, h, w, lb, ub, md, ratio, n_blocks, seed, t):
    """Ratios 0.25 / 0.3 (192 / 180 rows per sample on level 0 and 48 / 45 on level 1 at 16x16, 288 / 269 and 72 / 68 at 16x24:
    at 0.3 no multiple of 16, and odd) and 0.75 (nothing kept: the merged sequence is the dst rows alone)."""
    forward_with_tome_and_check(tome_unet, h, w, lb, ub, md, ratio, t, n_blocks, seed)


@pytest.mark.parametrize("h,w,lb,ub,md,ratio,n_blocks,seed,t", _cases("sd2"))
def test_sd2_shaped_unet_forward_with_tome_at_ratio_03(tome_sd2_unet, h, w, lb, ub, md, ratio, n_blocks, seed, t):
    forward_with_tome_and_check(tome_sd2_unet, h, w, lb, ub, md, ratio, t, n_blocks, seed)


def head_major(lib, cfg, C, heads, UB, Nm):
    """csrc/plan.hip, Builder::transformer: the q|k|v GEMM of a block stores K / V head-major, and attn_pipe40_kernel reads them
    at the offsets Mm C and 2 Mm C (Mm = UB Nm rows), when all of this holds."""
    Mm = UB * Nm
    return (C // heads == 40 and C % 160 == 0 and Nm % 128 == 0 and Nm >= 256 and lib.sd_op_gemm_tile_rows(Mm, 3 * C, 0) == 128
            and lib.sd_op_gemm_splitk(Mm, 3 * C, C, 0) == 1)


@pytest.mark.parametrize("h,w,lb,ub,md,ratio,n_blocks,seed,t", _cases("two_level"))
def test_unet_forward_with_tome_on_the_head_major_path(sdlib, tome_two_level_unet, h, w, lb, ub, md, ratio, n_blocks, seed, t):
    """32x32 latents on a 320 / 640 UNet: level 0 merges 1024 tokens to 512 (ratio 0.5) or 768 (0.25) rows per sample, and 16
    samples put the q|k|v GEMM on 128-row tiles, so the five level-0 blocks store K / V head-major.  With 8 latents under CFG the
    first block matches once per latent and runs on 8 samples -- 4096 / 6144 rows, 64-row tiles, token-major -- and the other
    four on 16: one plan holds both sides of the predicate."""
    cfg = tome_two_level_unet[0]
    C, heads = cfg.block_out_channels[0], cfg.num_heads
    Nm = h * w - to.num_merged(h * w, ratio)
    assert Nm == {0.5: 512, 0.25: 768}[ratio]
    assert sdlib.sd_op_gemm_tile_rows(16 * Nm, 3 * C, 0) == 128 and 16 * Nm > 8064 and sdlib.sd_op_gemm_tile_rows(8 * Nm, 3 * C, 0) == 64
    want = [head_major(sdlib, cfg, C, heads, lb if (i == 0 and ub == 2 * lb) else ub, Nm) for i in range(2)]
    assert want == [lb == 16, True]
    # the level-1 and mid blocks (C = 640, d = 80; 256 tokens -> 128 / 192 rows) never take it
    assert not head_major(sdlib, cfg, cfg.block_out_channels[1], heads, ub, 256 - to.num_merged(256, ratio))
    _, blocks = forward_with_tome_and_check(tome_two_level_unet, h, w, lb, ub, md, ratio, t, n_blocks, seed)
    assert [(b["h"], b["w"]) for b in blocks].count((32, 32)) == 5


@pytest.mark.parametrize("md", [1, 2])
@pytest.mark.parametrize("lb,ub", [(2, 4), (2, 2)])
@pytest.mark.parametrize("h,w", [(16, 16), (16, 24)])
def test_unet_forward_with_tome_matches_oracle_given_its_matchings(tome_unet, h, w, lb, ub, md):
    forward_with_tome_and_check(tome_unet, h, w, lb, ub, md)


def test_sd2_shaped_unet_forward_with_tome(tome_sd2_unet):
    forward_with_tome_and_check(tome_sd2_unet, 16, 16, 1, 2, 2)


def test_unet_off_is_off_and_deepcache_skip_plan_merges(tome_unet):
    cfg, sd, net, ocfg, _ = tome_unet
    lat, pe, ne = synth_inputs(cfg, 1)
    ctx = torch.cat([ne, pe]).cuda()
    net.set_deepcache(-1); net.set_tome(0.0)
    net.set_context(ctx)
    a = net.forward_latents(lat.cuda(), 2, 501.0).clone()
    net.set_tome(0.5, 1)
    net.set_context(ctx)
    on = net.forward_latents(lat.cuda(), 2, 501.0).clone()
    on2 = net.forward_latents(lat.cuda(), 2, 501.0).clone()
    net.set_tome(0.0)
    net.set_context(ctx)
    b = net.forward_latents(lat.cuda(), 2, 501.0).clone()
    assert torch.equal(a, b) and torch.equal(on, on2) and not torch.equal(a, on)
    # DeepCache branch 0: the skip step runs up_blocks.3.attentions.2 alone of the five merging blocks, and merges there -- it
    # partitions by the choice array set AFTER the full step, while the skipped first block keeps the full step's partition
    from sonicdiffusionbayeslab_amd.unet import CACHE_FULL_AND_STORE, CACHE_SKIP
    net.set_tome(0.5, 1)
    net.set_deepcache(0)
    net.set_context(ctx)
    g = torch.Generator().manual_seed(6)
    c1, c2 = (torch.randint(4, (5 * 64,), generator=g, dtype=torch.uint8) for _ in range(2))
    net.set_tome_choice(c1.cuda())
    full = net.forward_latents(lat.cuda(), 2, 501.0, cache_mode=CACHE_FULL_AND_STORE).clone()
    net.set_tome_choice(c2.cuda())
    skip = net.forward_latents(lat.cuda(), 2, 481.0, cache_mode=CACHE_SKIP).clone()
    torch.cuda.synchronize()
    first, last = net.tome_matching(0, 2)["tok"].long(), net.tome_matching(4, 2)["tok"].long()
    net.set_tome(0.0); net.set_deepcache(-1)
    assert torch.isfinite(full).all() and torch.isfinite(skip).all()
    assert torch.equal(first, torch.cat(to.partition(c1[:64], 16, 16))) and torch.equal(last, torch.cat(to.partition(c2[256:], 16, 16)))


# --------------------------------------------------------------------------------------------------------- pipelines
@pytest.fixture(scope="module")
def pipe():
    from sonicdiffusionbayeslab_amd.models import StableDiffusionModel
    from sonicdiffusionbayeslab_amd.registry import schedulers_registry
    from sonicdiffusionbayeslab_amd.weights import UNetConfig, make_synthetic_state_dict
    cfg = UNetConfig(sample_size=16)
    sd = to.tome_test_weights(make_synthetic_state_dict(cfg, seed=1234))
    model = StableDiffusionModel(unet_config=cfg, state_dict=dict(sd)).to("cuda:0")
    model.scheduler = schedulers_registry["ddim_scheduler"].from_config(model.scheduler.config)
    return cfg, model


def _call(model, cfg, steps=3, **kw):
    g = torch.Generator().manual_seed(29)
    lat = torch.randn((1, 4, 16, 16), generator=g)
    pe, ne = torch.randn((1, 77, 768), generator=g), torch.randn((1, 77, 768), generator=g)
    args = dict(prompt_embeds=pe, negative_prompt_embeds=ne, num_inference_steps=steps, guidance_scale=7.5, output_type="latent")
    if "image" not in kw:
        args["latents"] = lat
    args.update(kw)
    return model(**args)[0].images.float().cpu()


def test_pipeline_with_tome(pipe):
    """DDIM, three steps at 128x128 px.  Free-running parity against an oracle that matches on its own is NOT asserted: the
    library and the oracle may legitimately resolve a near-tie of two cosine similarities differently (the match is exact to
    4 C 2^-24, not bit-equal), which flips a merge and moves eps by more than a rounding; the UNet tests above feed the
    library's own matchings to the oracle instead."""
    cfg, model = pipe
    plain = _call(model, cfg)
    model.apply_tome(ratio=0.5, seed=3)
    a, b = _call(model, cfg), _call(model, cfg)
    assert torch.isfinite(a).all() and torch.equal(a, b)              # equal seeds: the same choices, the same result
    d = rel_l2(a, plain)
    print(f"[tome pipeline] 3-step DDIM with / without Token Merging: rel-L2 {d:.3f}")
    assert d > FREE_TOL
    model.apply_tome(ratio=0.5, seed=3, rand_every="call")
    c = _call(model, cfg)
    assert torch.isfinite(c).all() and torch.equal(c, _call(model, cfg)) and not torch.equal(c, a)
    model.apply_tome(ratio=0.5, seed=4)
    assert not torch.equal(_call(model, cfg), a)                       # another seed, other choices
    # under DeepCache and image-to-image
    from sonicdiffusionbayeslab_amd.deepcache import DeepCacheSDHelper
    model.apply_tome(ratio=0.5, seed=3)
    helper = DeepCacheSDHelper(pipe=model)
    helper.set_params(cache_interval=2, cache_branch_id=0)
    helper.enable()
    try:
        dc = _call(model, cfg, steps=4)
    finally:
        helper.disable()
    assert torch.isfinite(dc).all()
    img = torch.rand(1, 3, 128, 128, generator=torch.Generator().manual_seed(8))
    i2i = _call(model, cfg, steps=4, image=img, strength=0.5, generator=torch.Generator().manual_seed(1))
    assert torch.isfinite(i2i).all() and i2i.shape == (1, 4, 16, 16)
    # off is off: ratio 0 and remove_tome() give the model that never saw Token Merging, bit for bit
    model.apply_tome(ratio=0)
    assert torch.equal(_call(model, cfg), plain)
    model.apply_tome(ratio=0.25, max_downsample=2)
    assert not torch.equal(_call(model, cfg), plain)
    model.remove_tome()
    assert torch.equal(_call(model, cfg), plain)
