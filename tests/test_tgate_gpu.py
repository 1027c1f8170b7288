"""T-GATE on the GPU: the two kernels of csrc/tgate.hip bit for bit against torch on the CPU, their row partials against fp64
sums, the UNet's capturing and gated forwards against the patched oracle (tests/tgate_oracle.py), the handle's states, the
launch counts and the pipelines.

Bounds (a priori).
  h2, cache: fp32 sums of two bf16 values (exact or rounded once in fp32; the halving is exact) rounded once to nearest-even.
          torch on the CPU does the same arithmetic: the bound is EQUALITY of the bits.
  row partials: each is a sum of n fp32 terms (the stored bf16 h2 values, or their squares -- exact in the fused multiply-add) in
          some fixed tree: |err| <= (n - 1) 2^-24 sum|v| against the fp64 sum of the same stored values (v^2 for the squares).
  UNet: UNET_TOL = 2e-2 relative L2 against the oracle (tests/test_unet_gpu.py); the cache 1e-2 per block.
  loops: FREE_TOL / FREE_COS of tests/test_pipeline_gpu.py for a six-step DDIM loop."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from sonicdiffusionbayeslab_amd import _lib
from tests import tgate_oracle as tg
from tests.bounds import check_guards, forget_guards, guarded, guarded_input
from tests.util import cosine, rel_l2

UNET_TOL = 2e-2                     # tests/test_unet_gpu.py
FREE_TOL, FREE_COS = 6e-2, 0.998    # tests/test_pipeline_gpu.py
U32 = 2.0 ** -24
SHAPES = [(4, 320), (2 * 9 * 18, 1280), (3 * 100, 640), (1, 8), (2 * 64, 1280)]       # (cache rows, C)
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


# ------------------------------------------------------------------------------------------------------------ 1. kernels
def make_rows(rows, C, seed):
    """bf16 [rows, C]: noise, with the head of every row holding +-0, pairs whose exponents differ by more than 16 and exact
    ties of the bf16 rounding (placed by ``special``, at the same positions in both operands)."""
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(rows, C, generator=g) * 3.0).to(torch.bfloat16)


def special(a, b):
    """Columns 0..7 of (a, b): (+0, +0), (-0, -0), (+0, -0), (1, 2^-20), (-2^20, 1), (1, 2^-8) -- a tie, to even = 1 --,
    (1 + 2^-7, 2^-8) -- a tie, to even = 1 + 2^-6 --, (3, -3)."""
    va = [0.0, -0.0, 0.0, 1.0, -2.0 ** 20, 1.0, 1.0 + 2.0 ** -7, 3.0]
    vb = [0.0, -0.0, -0.0, 2.0 ** -20, 1.0, 2.0 ** -8, 2.0 ** -8, -3.0]
    a[:, :8] = torch.tensor(va, dtype=torch.bfloat16)
    b[:, :8] = torch.tensor(vb, dtype=torch.bfloat16)


def cpu_add(a, b):
    return (a.float() + b.float()).to(torch.bfloat16)


def bits(t):
    return t.contiguous().view(torch.int16)


def check_partials(rs, h2, what):
    """rs [2][M][2] against fp64 sums of the STORED h2 [M, C]: partial 0 = the first ceil(C / 16) 16-byte vectors of the row."""
    M, C = h2.shape
    nv = C // 8
    split = (nv + 1) // 2 * 8
    x = h2.double()
    for part, (lo, hi) in enumerate(((0, split), (split, C))):
        v, n = x[:, lo:hi], hi - lo
        for k, (ref, mag) in enumerate(((v.sum(1), v.abs().sum(1)), ((v * v).sum(1), (v * v).sum(1)))):
            err = (rs[part, :, k].double() - ref).abs()
            bound = max(n - 1, 0) * U32 * mag
            worst = (err - bound).max().item()
            print(f"[tgate partials] {what} part {part} {'sum' if k == 0 else 'sumsq'}: n = {n}, max err {err.max().item():.3e}, "
                  f"max err / bound {(err / bound.clamp_min(1e-300)).max().item() if n > 1 else 0.0:.3f}")
            assert worst <= 0.0, (what, part, k, worst)


def run_capture(sdlib, y, res, pair, with_stats=True):
    M, C = y.shape
    rows = M // pair
    yd, rd = guarded_input(y, label="y"), guarded_input(res, label="res")
    h2 = guarded((M, C), torch.bfloat16, label="h2")
    cache = guarded((rows, C), torch.bfloat16, label="cache")
    rs = guarded((2, M, 2), torch.float32, label="rowstats") if with_stats else None
    _lib.check(sdlib.sd_op_tgate_capture(stream(), P(yd), P(rd), P(h2), P(cache), _lib.ptr(rs), rows, C, pair), "sd_op_tgate_capture")
    torch.cuda.synchronize()
    assert torch.equal(bits(yd.cpu()), bits(y)) and torch.equal(bits(rd.cpu()), bits(res))          # the inputs are never modified
    return h2.cpu(), cache.cpu(), None if rs is None else rs.cpu()


def run_apply(sdlib, h1, cache, with_stats=True):
    M, C = h1.shape
    hd, cd = guarded_input(h1, label="h1"), guarded_input(cache, label="cache")
    h2 = guarded((M, C), torch.bfloat16, label="h2")
    rs = guarded((2, M, 2), torch.float32, label="rowstats") if with_stats else None
    _lib.check(sdlib.sd_op_tgate_apply(stream(), P(hd), P(cd), P(h2), _lib.ptr(rs), M, C), "sd_op_tgate_apply")
    torch.cuda.synchronize()
    assert torch.equal(bits(hd.cpu()), bits(h1)) and torch.equal(bits(cd.cpu()), bits(cache))
    return h2.cpu(), None if rs is None else rs.cpu()


@pytest.mark.parametrize("pair", [1, 2])
@pytest.mark.parametrize("rows,C", SHAPES, ids=[f"{r}x{c}" for r, c in SHAPES])
def test_capture_is_bit_exact_with_guard_bands_partials_and_determinism(sdlib, rows, C, pair):
    M = rows * pair
    y, res = make_rows(M, C, 100 + C), make_rows(M, C, 200 + C)
    special(y, res)
    if pair == 2:       # the pair mean's own ties and zeros: (1, 1 + 2^-7) / 2 = 1 + 2^-8 -> 1; (-0, -0) -> -0; (+0, -0) -> +0
        y[rows:, :8] = torch.tensor([-0.0, -0.0, 0.0, 1.0 + 2.0 ** -7, 1.0, 2.0 ** -20, 3.0, -3.0], dtype=torch.bfloat16)
        y[:rows, 3] = 1.0
    h2, cache, rs = run_capture(sdlib, y, res, pair)
    check_guards()                                                         # (the capture writes exactly `rows` cache rows)
    want_cache = ((y[:rows].float() + y[rows:].float()) * 0.5).to(torch.bfloat16) if pair == 2 else y
    assert torch.equal(bits(h2), bits(cpu_add(res, y))), "h2"
    assert torch.equal(bits(cache), bits(want_cache)), "cache"
    check_partials(rs, h2, f"capture {M}x{C} pair {pair}")
    h2b, cacheb, rsb = run_capture(sdlib, y, res, pair)
    assert torch.equal(bits(h2b), bits(h2)) and torch.equal(bits(cacheb), bits(cache)) and torch.equal(rsb.view(torch.int32), rs.view(torch.int32))
    h2c, cachec, _ = run_capture(sdlib, y, res, pair, with_stats=False)      # without partials: the same rows
    assert torch.equal(bits(h2c), bits(h2)) and torch.equal(bits(cachec), bits(cache))
    check_guards()


@pytest.mark.parametrize("rows,C", SHAPES, ids=[f"{r}x{c}" for r, c in SHAPES])
def test_apply_is_bit_exact_with_guard_bands_partials_and_determinism(sdlib, rows, C):
    h1, cache = make_rows(rows, C, 300 + C), make_rows(rows, C, 400 + C)
    special(h1, cache)
    h2, rs = run_apply(sdlib, h1, cache)
    check_guards()
    assert torch.equal(bits(h2), bits(cpu_add(h1, cache)))
    check_partials(rs, h2, f"apply {rows}x{C}")
    h2b, rsb = run_apply(sdlib, h1, cache)
    assert torch.equal(bits(h2b), bits(h2)) and torch.equal(rsb.view(torch.int32), rs.view(torch.int32))
    assert torch.equal(bits(run_apply(sdlib, h1, cache, with_stats=False)[0]), bits(h2))
    check_guards()


def test_the_partials_sum_to_the_row_moments_a_layernorm_needs(sdlib):
    """The format contract of GemmArgs::ln_rs: the partials of a row add up to its sum and sum of squares, i.e. to the mean and
    variance LayerNorm normalises with."""
    rows, C = 256, 320
    h1, cache = make_rows(rows, C, 1), make_rows(rows, C, 2)
    h2, rs = run_apply(sdlib, h1, cache)
    x = h2.double()
    s, q = rs[:, :, 0].double().sum(0), rs[:, :, 1].double().sum(0)
    assert torch.allclose(s, x.sum(1), rtol=0, atol=C * U32 * float(x.abs().sum(1).max()))
    assert torch.allclose(q, (x * x).sum(1), rtol=0, atol=C * U32 * float((x * x).sum(1).max()))
    mean, var = s / C, q / C - (s / C) ** 2
    assert torch.allclose(mean, x.mean(1), atol=1e-5) and torch.allclose(var, x.var(1, unbiased=False), rtol=1e-4, atol=1e-5)


def test_refusals_write_nothing(sdlib):
    rows, C = 4, 320
    y, res = make_rows(2 * rows, C, 5), make_rows(2 * rows, C, 6)
    yd, rd = guarded_input(y), guarded_input(res)
    h2, cache = guarded((2 * rows, C), torch.bfloat16), guarded((rows, C), torch.bfloat16)

    def refused(rc, *needles):
        assert rc != 0
        msg = sdlib.sd_last_error().decode()
        assert all(n in msg for n in needles), msg
    s = stream()
    refused(sdlib.sd_op_tgate_capture(s, P(yd), P(rd), P(h2), P(cache), None, rows, 324, 2), "tgate_capture", "C=324")
    refused(sdlib.sd_op_tgate_capture(s, P(yd), P(rd), P(h2), P(cache), None, rows, C, 3), "pair=3")
    refused(sdlib.sd_op_tgate_capture(s, P(yd), P(rd), P(h2), None, None, rows, C, 2), "tgate_capture: null")
    refused(sdlib.sd_op_tgate_capture(s, None, P(rd), P(h2), P(cache), None, rows, C, 2), "tgate_capture: null")
    refused(sdlib.sd_op_tgate_capture(s, P(yd), P(rd), P(yd), P(cache), None, rows, C, 2), "new tensors")
    refused(sdlib.sd_op_tgate_apply(s, P(yd), P(rd), P(h2), None, rows, 12), "tgate_apply", "C=12")
    refused(sdlib.sd_op_tgate_apply(s, P(yd), None, P(h2), None, rows, C), "tgate_apply: null")
    refused(sdlib.sd_op_tgate_apply(s, P(yd), P(rd), P(h2), None, 0, C), "rows=0")
    torch.cuda.synchronize()
    assert torch.isnan(h2).all() and torch.isnan(cache).all()              # nothing was written
    check_guards()


# ------------------------------------------------------------------------------------------------------- 2. UNet forward
_NETS = {}


def net_of(name):
    from sonicdiffusionbayeslab_amd.unet import HipUNet2DConditionModel
    if name not in _NETS:
        cfg, sd, ocfg, heads = tg.env(name)
        _NETS[name] = HipUNet2DConditionModel(cfg, sd)
    return _NETS[name]


def gpu_capture_and_gated(case, net=None):
    """(eps of the capturing forward, eps of the gated forward, the cache slices as fp32 CPU tensors) of the library."""
    _, name, h, w, lb, cfg_on, _, t0, t1 = case
    net = net or net_of(name)
    lat0, lat1, ctx = tg.inputs(case)
    ub = ctx.shape[0]
    net.set_deepcache(-1)
    try:
        net.set_tgate(net.TGATE_CAPTURE, lb, h, w)
        net.set_context(ctx.cuda(), h, w)
        cap = net.forward_latents(lat0.cuda(), ub, t0).clone()
        net.set_tgate(net.TGATE_REUSE, lb, h, w)
        gated = net.forward_latents(lat1.cuda(), lb, t1).clone()
        torch.cuda.synchronize()
        n = len(net.tgate_blocks(lb, h, w))
        slices = [net.tgate_cache_block(i, lb, h, w).float().cpu() for i in range(n)]
    finally:
        net.set_tgate(net.TGATE_OFF)
    return cap.cpu(), gated.cpu(), slices


@pytest.mark.parametrize("case", tg.CASES, ids=[c[0] for c in tg.CASES])
def test_capturing_and_gated_forwards_match_the_oracle(case):
    _, name, h, w, lb, cfg_on, _, _, _ = case
    cap, gated, slices = gpu_capture_and_gated(case)
    ref = tg.reference(case)
    e_cap, e_gated = rel_l2(cap, ref["capture"]), rel_l2(gated, ref["gated"])
    plain = tg.variant_forward(case, "plain")
    print(f"[tgate unet] {case[0]}: capturing forward vs the plain oracle {e_cap:.3e}; gated forward vs the patched oracle {e_gated:.3e}; "
          f"gated vs the plain cond oracle {rel_l2(gated, plain):.3f} (the oracle's own {rel_l2(ref['gated'], plain):.3f})")
    assert torch.isfinite(cap).all() and e_cap < UNET_TOL
    assert torch.isfinite(gated).all() and e_gated < UNET_TOL
    assert rel_l2(gated, plain) > tg.FLOOR
    st = ref["state"]
    prefixes = tg.block_prefixes(tg.env(name)[0])
    assert len(slices) == len(prefixes)
    worst = 0.0
    for p, got in zip(prefixes, slices):
        want = st.cache[p]
        assert got.shape == (want.shape[0] * want.shape[1], want.shape[2]), (p, got.shape, want.shape)
        worst = max(worst, rel_l2(got, want.reshape(got.shape)))
    print(f"[tgate unet] {case[0]}: worst cache slice rel-L2 {worst:.3e} over {len(slices)} blocks")
    assert worst < tg.CACHE_TOL


def plain_forward(net, case):
    _, name, h, w, lb, _, _, t0, _ = case
    lat0, _, ctx = tg.inputs(case)
    net.set_deepcache(-1)
    net.set_context(ctx.cuda(), h, w)
    eps = net.forward_latents(lat0.cuda(), ctx.shape[0], t0).clone()
    torch.cuda.synchronize()
    return eps.cpu()


def test_off_after_on_is_bit_equal_to_a_fresh_handle():
    from sonicdiffusionbayeslab_amd.unet import HipUNet2DConditionModel
    case = tg.CASES[2]                     # two_level: the smallest set of weights
    cfg, sd, _, _ = tg.env(case[1])
    fresh = HipUNet2DConditionModel(cfg, sd)
    never = plain_forward(fresh, case)                                     # a handle that never saw T-GATE
    net = net_of(case[1])
    gpu_capture_and_gated(case, net)
    assert torch.equal(plain_forward(net, case), never)
    plans = fresh.plan_count()
    gpu_capture_and_gated(case, fresh)
    assert fresh.plan_count() > plans                                      # the capture and the reuse plans are plans of their own
    assert torch.equal(plain_forward(fresh, case), never) and fresh.plan_count() > plans


def test_reuse_before_capture_and_at_another_batch_fail_by_name():
    case = tg.CASES[0]
    _, name, h, w, lb, _, _, t0, t1 = case
    net = net_of(name)
    lat0, lat1, ctx = tg.inputs(case)
    net.set_deepcache(-1)
    try:
        with pytest.raises(_lib.SdHipError, match="reuse before any capture"):
            net.set_tgate(net.TGATE_REUSE, lb, h, w)
        net.set_tgate(net.TGATE_CAPTURE, lb, h, w)
        with pytest.raises(_lib.SdHipError, match="reuse before any capture"):      # capture mode set, but no forward ran
            net.set_tgate(net.TGATE_REUSE, lb, h, w)
        net.set_tgate(net.TGATE_CAPTURE, lb, h, w)
        net.set_context(ctx.cuda(), h, w)
        with pytest.raises(_lib.SdHipError, match="latent batch or twice it"):
            net.set_context(torch.cat([ctx, ctx[:2]]).cuda(), h, w)
            net.forward_latents(torch.cat([lat0, lat0, lat0]).cuda(), 6, t0)
        net.set_context(ctx.cuda(), h, w)
        net.forward_latents(lat0.cuda(), ctx.shape[0], t0)
        with pytest.raises(_lib.SdHipError, match=rf"reuse for 1 latents at {h}x{w}, but the capture filled its buffer for {lb} latents"):
            net.set_tgate(net.TGATE_REUSE, 1, h, w)
        with pytest.raises(_lib.SdHipError, match="but the capture filled its buffer"):
            net.set_tgate(net.TGATE_REUSE, lb, h, w - 8)
        net.set_tgate(net.TGATE_REUSE, lb, h, w)                              # the failed calls changed nothing
        with pytest.raises(_lib.SdHipError, match="runs at the batch of the capture's latents"):
            net.forward_latents(lat1.cuda(), 2 * lb, t1)
        with pytest.raises(_lib.SdHipError, match="T-GATE reuse mode"):
            net.set_context(ctx.cuda(), h, w)
        assert torch.isfinite(net.forward_latents(lat1.cuda(), lb, t1)).all()
    finally:
        net.set_tgate(net.TGATE_OFF)


@pytest.mark.parametrize("name,blocks,fused", [("sd15", 16, 0), ("two_level", 11, 5)])
def test_the_profile_kinds_count_the_launches(name, blocks, fused):
    cfg = tg.env(name)[0]
    net = net_of(name)
    s, lb = cfg.sample_size, 2
    g = torch.Generator().manual_seed(3)
    lat, ctx = torch.randn(lb, 4, s, s, generator=g).cuda(), torch.randn(2 * lb, cfg.context_len, cfg.cross_attention_dim, generator=g).cuda()
    net.set_deepcache(-1)
    net.set_context(ctx)
    plain = net.forward_profiled(lat, 2 * lb, 500.0)
    assert "tgate_capture" not in plain and "tgate_apply" not in plain and "tgate_zero" not in plain
    try:
        net.set_tgate(net.TGATE_CAPTURE, lb)
        net.set_context(ctx)
        cap = net.forward_profiled(lat, 2 * lb, 500.0)
        net.set_tgate(net.TGATE_REUSE, lb)
        gated = net.forward_profiled(lat, lb, 480.0)
    finally:
        net.set_tgate(net.TGATE_OFF)
    assert cap["tgate_capture"]["launches"] == blocks and cap["tgate_capture"]["bytes"] > 0 and "tgate_apply" not in cap
    assert cap.get("xattn_fused", {"launches": 0})["launches"] == fused == plain.get("xattn_fused", {"launches": 0})["launches"]
    assert ("tgate_zero" in cap) == (fused > 0)
    assert cap["attention"]["launches"] == plain["attention"]["launches"] and cap["gemm"]["launches"] == plain["gemm"]["launches"]
    assert gated["tgate_apply"]["launches"] == blocks and gated["tgate_apply"]["bytes"] > 0 and "tgate_capture" not in gated
    # no cross-attention launch in the gated plan: the attention kernel runs for attn1 alone, the fused form not at all, and
    # every block lost its cross-attention GEMMs
    assert "xattn_fused" not in gated and "tgate_zero" not in gated
    assert gated["attention"]["launches"] == blocks
    assert gated["gemm"]["launches"] <= plain["gemm"]["launches"] - (blocks - fused)
    assert gated["layernorm"]["launches"] <= plain["layernorm"]["launches"]


def test_with_token_merging_and_freeu_the_gated_forward_continues_the_capture():
    """Token Merging (ratio 0.5, fixed dst choice) and FreeU on, no CFG: the cache then holds exactly the y of the capturing
    forward, so a gated forward on the SAME latents and timestep repeats that forward up to the roundings of the two plans; and
    the capturing forward is the plain forward of the same settings up to the one extra rounding of y."""
    from tests import freeu_oracle as fo
    case = tg.CASES[4]
    _, name, h, w, lb, _, _, t0, _ = case
    net = net_of(name)
    lat0, _, ctx = tg.inputs(case)
    net.set_deepcache(-1)
    net.set_tome(0.5, 1)
    net.set_freeu(*fo.GIVEN)
    try:
        net.set_context(ctx.cuda(), h, w)
        plain = net.forward_latents(lat0.cuda(), lb, t0).clone().cpu()
        net.set_tgate(net.TGATE_CAPTURE, lb, h, w)
        net.set_context(ctx.cuda(), h, w)
        cap = net.forward_latents(lat0.cuda(), lb, t0).clone().cpu()
        net.set_tgate(net.TGATE_REUSE, lb, h, w)
        gated = net.forward_latents(lat0.cuda(), lb, t0).clone().cpu()
        net.set_tgate(net.TGATE_OFF)
        net.set_tome(0.0)
        net.disable_freeu()
        net.set_context(ctx.cuda(), h, w)
        bare = net.forward_latents(lat0.cuda(), lb, t0).clone().cpu()
    finally:
        net.set_tgate(net.TGATE_OFF)
        net.set_tome(0.0)
        net.disable_freeu()
    print(f"[tgate + tome + freeu] capture vs plain {rel_l2(cap, plain):.3e}; gated vs capture {rel_l2(gated, cap):.3e}; with / "
          f"without ToMe and FreeU {rel_l2(plain, bare):.3f}")
    assert torch.isfinite(gated).all()
    assert rel_l2(cap, plain) < UNET_TOL and rel_l2(gated, cap) < UNET_TOL
    assert rel_l2(plain, bare) > 10 * UNET_TOL                             # both settings were on


def test_the_state_can_be_set_while_the_workspace_key_is_dropped():
    """``set_tome``, ``set_deepcache`` and ``reserve_tgate`` drop the workspace key and keep the workspace until the next
    ``set_context``: ``set_tgate`` in between must not read the key."""
    case = tg.CASES[4]
    _, name, h, w, lb, _, _, t0, _ = case
    net = net_of(name)
    lat0, _, ctx = tg.inputs(case)
    net.set_deepcache(-1)
    net.set_context(ctx.cuda(), h, w)
    plain = net.forward_latents(lat0.cuda(), lb, t0).clone()
    try:
        net.set_tome(0.5, 1)
        assert net._ws is not None and net._ws_key is None
        net.set_tgate(net.TGATE_OFF)
        net.set_tgate(net.TGATE_CAPTURE, lb, h, w)
        net.set_tgate(net.TGATE_OFF)
    finally:
        net.set_tgate(net.TGATE_OFF)
        net.set_tome(0.0)
    net.set_context(ctx.cuda(), h, w)
    assert torch.equal(net.forward_latents(lat0.cuda(), lb, t0), plain)


# ---------------------------------------------------------------------------------------------------------- 3. pipelines
@pytest.fixture(scope="module")
def pipe():
    from sonicdiffusionbayeslab_amd.models import StableDiffusionModel
    from sonicdiffusionbayeslab_amd.registry import schedulers_registry
    cfg, sd, ocfg, _ = tg.env("sd15")
    model = StableDiffusionModel(unet_config=cfg, state_dict=dict(sd)).to("cuda:0")
    model.scheduler = schedulers_registry["ddim_scheduler"].from_config(model.scheduler.config)
    return cfg, sd, ocfg, model


def _call(model, steps=6, gs=7.5):
    g = torch.Generator().manual_seed(29)
    lat = torch.randn((1, 4, 16, 16), generator=g)
    pe, ne = torch.randn((1, 77, 768), generator=g), torch.randn((1, 77, 768), generator=g)
    out = model(prompt_embeds=pe, negative_prompt_embeds=ne, latents=lat, num_inference_steps=steps, guidance_scale=gs,
                output_type="latent")[0].images.float().cpu()
    return out, (lat, pe, ne)


def test_the_gated_loop_matches_the_oracle_loop_and_off_is_off(pipe):
    from oracle.schedulers import DDIMOracle
    cfg, sd, ocfg, model = pipe
    plain, (lat, pe, ne) = _call(model)
    assert model.enable_tgate(3) is model
    on, _ = _call(model)
    with torch.no_grad():
        ref = tg.sample_loop(sd, ocfg, DDIMOracle(), pe, ne, lat, 6, 7.5, 3)
        ref_plain = tg.sample_loop(sd, ocfg, DDIMOracle(), pe, ne, lat, 6, 7.5, 6)
    err, cs, moved, own = rel_l2(on, ref), cosine(on, ref), rel_l2(on, plain), rel_l2(ref, ref_plain)
    print(f"[tgate model] 6-step DDIM, gate 3: rel-L2 vs the oracle loop {err:.3e} cos {cs:.5f}; gated vs plain {moved:.3f} (the "
          f"oracle's own {own:.3f}); plain vs its oracle {rel_l2(plain, ref_plain):.3e}")
    assert torch.isfinite(on).all() and err < FREE_TOL and cs > FREE_COS
    # the oracle's own gated / plain distance at this length is 0.047, below FREE_TOL: what tells a loop that gated from one
    # that never did is being nearer to the gated oracle than to the plain one -- err < own / 2 puts the result on the gated
    # side of the midpoint (triangle inequality: its distance to the plain oracle is then > own / 2 > err)
    assert own > 2 * UNET_TOL and err < own / 2 and rel_l2(on, ref_plain) > own / 2 and moved > 0
    again, _ = _call(model)
    assert torch.equal(again, on)
    model.enable_tgate(6)                                                  # a gate at the step count: the plain loop
    assert torch.equal(_call(model)[0], plain)
    model.enable_tgate(9)
    assert torch.equal(_call(model)[0], plain)
    assert model.disable_tgate() is model
    assert torch.equal(_call(model)[0], plain)


def test_the_gated_loop_without_cfg_and_with_dpm_solver_history(pipe):
    """guidance 1 (pair = 1), and DPM-Solver++ order 2 across the gate: its history holds combined predictions at the latent
    batch on both sides of the gate."""
    from oracle.schedulers import DDIMOracle, DPMSolverOracle
    from sonicdiffusionbayeslab_amd.registry import schedulers_registry
    cfg, sd, ocfg, model = pipe
    model.enable_tgate(3)
    try:
        on, (lat, pe, ne) = _call(model, gs=1.0)
        with torch.no_grad():
            ref = tg.sample_loop(sd, ocfg, DDIMOracle(), pe, None, lat, 6, 1.0, 3)
        print(f"[tgate model] no CFG: rel-L2 vs the oracle loop {rel_l2(on, ref):.3e}")
        assert rel_l2(on, ref) < FREE_TOL and cosine(on, ref) > FREE_COS
        kw = dict(solver_order=2, algorithm_type="dpmsolver++", final_sigmas_type="zero")
        ddim = model.scheduler
        from sonicdiffusionbayeslab_amd.schedulers import PNDMConfigStub
        model.scheduler = schedulers_registry["dpm_solver_scheduler"].from_config(PNDMConfigStub().config, **kw)
        try:
            on, _ = _call(model)
        finally:
            model.scheduler = ddim
        with torch.no_grad():
            ref = tg.sample_loop(sd, ocfg, DPMSolverOracle(**kw), pe, ne, lat, 6, 7.5, 3)
        print(f"[tgate model] DPM-Solver++ 2: rel-L2 vs the oracle loop {rel_l2(on, ref):.3e}")
        assert rel_l2(on, ref) < FREE_TOL and cosine(on, ref) > FREE_COS
    finally:
        model.disable_tgate()


def _handle_loop(net, lat, pe, ne, steps, gs, gate):
    """``tgate_oracle.sample_loop`` with the library's UNet handle in place of the oracle's UNet: the oracle's DDIM steps on the
    host, the guidance in torch, the handle's state set by hand.  It shares no line with ``_sample``.  The settings already on
    the handle (Token Merging, FreeU) stay."""
    from oracle.schedulers import DDIMOracle
    sch = DDIMOracle()
    sch.set_timesteps(steps)
    ts = list(sch.timesteps)
    ctx = torch.cat([ne, pe]).cuda()
    lb, (h, w) = lat.shape[0], lat.shape[2:]
    x = lat.float() * sch.init_noise_sigma
    g = gate if gate is not None and gate < len(ts) else None
    net.set_context(ctx, h, w)
    try:
        for i, t in enumerate(ts):
            if g is not None and i == g - 1:
                net.set_tgate(net.TGATE_CAPTURE, lb, h, w)
                net.set_context(ctx, h, w)
            if g is not None and i == g:
                net.set_tgate(net.TGATE_REUSE, lb, h, w)
            xi = sch.scale_model_input(x, t).cuda()
            if g is not None and i >= g:
                eps = net.forward_latents(xi, lb, float(t)).cpu()
            else:
                u, c = net.forward_latents(xi, 2 * lb, float(t)).cpu().chunk(2)
                eps = u + gs * (c - u)
            x = sch.step(eps, t, x, return_dict=False)[0]
    finally:
        net.set_tgate(net.TGATE_OFF)
    return x


def test_the_gated_loop_with_token_merging_and_freeu(pipe):
    """No oracle loop exists with Token Merging in it (its matchings flip on roundings, so the oracle takes the library's own per
    forward).  The reference is therefore ``_handle_loop``: the oracle's loop and scheduler around the library's forwards, whose
    capture and reuse under Token Merging and FreeU the UNet test above checks.  What this test adds is the loop: ``_sample`` must
    gate at the same step, at the same batch, with a fresh capture and without guidance behind the gate.  Bounds: FREE_TOL /
    FREE_COS, the tolerance of a six-step loop, and, as in the main loop test, the result must lie on the gated side of the
    midpoint between the gated and the plain reference.  Measured on an MI355X: 1.87e-2 from the gated reference (the plain call
    is 1.95e-2 from the plain one: the pipeline's own step arithmetic), the references 0.058 apart."""
    from tests import freeu_oracle as fo
    cfg, sd, ocfg, model = pipe
    model.apply_tome(0.5, use_rand=False)
    model.enable_freeu(*fo.GIVEN)
    try:
        plain, (lat, pe, ne) = _call(model)
        model.enable_tgate(3)
        on, _ = _call(model)
        model.enable_tgate(6)
        same, _ = _call(model)
        model.disable_tgate()
        ref = _handle_loop(model.unet, lat, pe, ne, 6, 7.5, 3)             # (the handle still has both settings on)
        ref_plain = _handle_loop(model.unet, lat, pe, ne, 6, 7.5, None)
    finally:
        model.disable_tgate()
        model.remove_tome()
        model.disable_freeu()
    bare, _ = _call(model)
    err, cs, own = rel_l2(on, ref), cosine(on, ref), rel_l2(ref, ref_plain)
    print(f"[tgate model] Token Merging + FreeU, 6-step DDIM, gate 3: rel-L2 vs the handle loop {err:.3e} cos {cs:.5f}; plain vs "
          f"its handle loop {rel_l2(plain, ref_plain):.3e}; gated vs plain {rel_l2(on, plain):.3f} (the reference's own {own:.3f}); "
          f"with / without ToMe and FreeU {rel_l2(plain, bare):.3f}")
    assert torch.isfinite(on).all() and err < FREE_TOL and cs > FREE_COS
    assert rel_l2(plain, ref_plain) < FREE_TOL
    assert err < own / 2 and rel_l2(on, ref_plain) > own / 2               # on the gated side of the midpoint
    assert rel_l2(plain, bare) > FREE_TOL                                  # both settings were on
    assert torch.equal(same, plain)
