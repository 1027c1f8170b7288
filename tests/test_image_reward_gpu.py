"""ImageReward on libsdhip: the masked attention kernel and the reward head per element, the tiny model end to end against the
recorded transformers golden and the fp32 oracle, the v1.0 shape against the oracle, the win-rate metric and the validate
wiring.

Gates.  Attention: tests/bounds.attention_ref_bound per element (a priori), applied per sample to the gathered valid keys.
Reward head: fp64 dot product, fp32 accumulation bound.  Model: the project's tower gate TOL = 1.5e-2 rel-L2 on the features
PER SAMPLE (tests/test_clip_gpu.py), and rewards within tol_r = TOL ||f_ref|| ||w_fold|| / std, which is what a feature error of
TOL can move the folded head's output by.  Win-rate and rank decisions are those whose oracle gap exceeds 2 tol_r
(tests/test_image_reward_cpu.py::test_gap_condition_of_the_gpu_decisions)."""
import json
import math
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

from sonicdiffusionbayeslab_amd import _lib
from sonicdiffusionbayeslab_amd import image_reward as IR
from tests import image_reward_oracle as O
from tests import image_reward_util as U
from tests.bounds import (ATOL_TINY, U32, assert_elementwise, attention_ref_bound, check_guards, guarded, guarded_input,
                          heads_view)
from tests.util import rel_l2

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "image_reward_golden.json")
TOL = U.TOL


# ---- sd_op_bert_attention ---------------------------------------------------------------------------------------------

def _masks(B, Lk, kind):
    """int32 [B][Lk] or None.  "lens": prefixes of mixed valid lengths; "holes": valid keys scattered, not a prefix."""
    if kind is None:
        return None
    m = torch.zeros(B, Lk, dtype=torch.int32)
    if kind == "holes":
        g = torch.Generator().manual_seed(Lk)
        m = (torch.rand(B, Lk, generator=g) < 0.6).int()
        m[:, Lk // 2] = 1                                       # (every sample keeps a key)
        m[:, 0] = 0
        return m
    for b, n in enumerate(kind):
        m[b, :n] = 1
    return m


# (B, heads, Lq, Lk, mask kind, the fold's strided K|V layout)
ATTN_CASES = [
    (1, 1, 1, 1, None, False),
    (3, 3, 3, 197, None, True),
    (1, 3, 16, 33, "holes", False),
    (3, 1, 16, 33, "holes", True),
    (5, 3, 35, 35, (2, 15, 16, 17, 35), False),
    (5, 1, 35, 35, (35, 17, 16, 15, 2), True),
    (3, 3, 35, 197, None, True),
    (1, 1, 35, 197, None, False),
    (3, 3, 64, 320, "holes", True),
    (1, 1, 64, 320, None, False),
]


@pytest.mark.parametrize("case", ATTN_CASES, ids=lambda c: f"B{c[0]}h{c[1]}q{c[2]}k{c[3]}{'m' if c[4] else ''}{'s' if c[5] else ''}")
def test_bert_attention_per_element(sdlib, case):
    B, heads, Lq, Lk, kind, strided = case
    H = 64 * heads
    g = torch.Generator().manual_seed(B * 1000 + heads * 100 + Lq + Lk)
    q = (torch.randn(B * Lq, H, generator=g) * 1.5).to(torch.bfloat16)
    k = (torch.randn(B * Lk, H, generator=g) * 1.5).to(torch.bfloat16)
    v = (torch.randn(B * Lk, H, generator=g) * 1.5).to(torch.bfloat16)
    mask = _masks(B, Lk, kind)
    kd, vd = k.clone(), v.clone()
    if mask is not None:                                        # masked rows hold huge finite values of both signs
        dead = (mask.reshape(-1) == 0)
        sign = torch.where(torch.arange(H) % 2 == 0, 1.0, -1.0).to(torch.bfloat16)
        kd[dead] = 3e38 * sign
        vd[dead] = -3e38 * sign
    if strided:        # the one-GEMM K|V layout: [B Lk][layers 2 H] with this layer's k | v at a non-zero column offset
        ldkv, koff = 3 * 2 * H, 2 * H
        buf = (torch.randn(B * Lk, ldkv, generator=g) * 1.5).to(torch.bfloat16)
        buf[:, koff:koff + H] = kd
        buf[:, koff + H:koff + 2 * H] = vd
        kv = guarded_input(buf, label="k|v of all layers")
        kp, vp = kv.data_ptr() + koff * 2, kv.data_ptr() + (koff + H) * 2
    else:
        ldkv = H
        kp, vp = guarded_input(kd, label="k").data_ptr(), guarded_input(vd, label="v").data_ptr()
    qd = guarded_input(q, label="q")
    md = guarded_input(mask, label="mask") if mask is not None else None
    out = guarded((B * Lq, H), torch.bfloat16, label="out")
    _lib.check(sdlib.sd_op_bert_attention(_lib.current_stream(), qd.data_ptr(), H, kp, vp, ldkv, _lib.ptr(md), out.data_ptr(), H,
                                          B, heads, Lq, Lk), "sd_op_bert_attention")
    torch.cuda.synchronize()
    got = heads_view(out.cpu().float().view(B, Lq, H), B, Lq, heads, 64)
    qh = heads_view(q.float().view(B, Lq, H), B, Lq, heads, 64)
    kh = heads_view(k.float().view(B, Lk, H), B, Lk, heads, 64)
    vh = heads_view(v.float().view(B, Lk, H), B, Lk, heads, 64)
    for b in range(B):                                           # per sample: the reference sees the valid keys only
        keep = torch.arange(Lk) if mask is None else torch.nonzero(mask[b]).flatten()
        ref, bound = attention_ref_bound(qh[b:b + 1], kh[b:b + 1][:, :, keep], vh[b:b + 1][:, :, keep], 1.0 / math.sqrt(64))
        assert_elementwise(got[b:b + 1], ref, bound, f"bert attention {case} sample {b} ({len(keep)} valid keys)",
                           ("b", "head", "row", "d"))
    check_guards()


def test_bert_attention_refusals_launch_nothing(sdlib):
    H = 64
    q = guarded_input(torch.zeros(65, H, dtype=torch.bfloat16), label="q")
    kv = guarded_input(torch.zeros(2 * 321, H, dtype=torch.bfloat16), label="kv")
    out = guarded((2 * 65, H), torch.bfloat16, label="out")
    s = _lib.current_stream()

    def call(B, Lq, Lk, mask):
        return sdlib.sd_op_bert_attention(s, q.data_ptr(), H, kv.data_ptr(), kv.data_ptr(), H, _lib.ptr(mask), out.data_ptr(), H, B, 1,
                                          Lq, Lk)

    for args, word in (((1, 65, 8, None), "Lq=65"), ((1, 8, 321, None), "Lk=321"), ((1, 0, 8, None), "Lq=0")):
        with pytest.raises(_lib.SdHipError, match=word):
            _lib.check(call(*args))
    m = torch.ones(2, 8, dtype=torch.int32)
    m[1] = 0
    with pytest.raises(_lib.SdHipError, match="sample 1 has no valid key"):
        _lib.check(call(2, 8, 8, guarded_input(m, label="mask")))
    torch.cuda.synchronize()
    assert torch.isnan(out.float()).all()                        # nothing ran: the output still holds its fill
    check_guards()


# ---- sd_op_reward_head ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("B,H", [(1, 128), (5, 128), (1, 768), (5, 768)])
def test_reward_head_per_element(sdlib, B, H):
    g = torch.Generator().manual_seed(B * 1000 + H)
    L = 3                                                        # the class-token row is row 0 of every L-row sample
    hid = (torch.randn(B * L, H, generator=g) * 2).to(torch.bfloat16)
    w = torch.randn(H, generator=g) / math.sqrt(H)
    bias = torch.randn(1, generator=g)
    mean, std = IR.REWARD_MEAN, IR.REWARD_STD
    rewards = guarded((B,), torch.float32, label="rewards")
    feats = guarded((B, H), torch.float32, label="features")
    _lib.check(sdlib.sd_op_reward_head(_lib.current_stream(), guarded_input(hid, label="hidden").data_ptr(), L * H,
                                       guarded_input(w, label="w").data_ptr(), guarded_input(bias, label="bias").data_ptr(), mean,
                                       std, B, H, rewards.data_ptr(), feats.data_ptr()), "sd_op_reward_head")
    torch.cuda.synchronize()
    x = hid.view(B, L, H)[:, 0].double()
    assert torch.equal(feats.cpu(), x.float())
    dot = x @ w.double()
    mag = x.abs() @ w.double().abs() + abs(float(bias))
    ref = (dot + float(bias) - float(torch.tensor(mean, dtype=torch.float32))) / float(torch.tensor(std, dtype=torch.float32))
    # fp32 accumulation of H terms in any order, the bias / mean adds and the division: (H + 4) u on the magnitudes
    bound = ((H + 4) * U32 * (mag + abs(mean)) / std + ATOL_TINY)
    assert_elementwise(rewards.cpu(), ref, bound, f"reward head B={B} H={H}", ("b",))
    # rewards only
    r2 = guarded((B,), torch.float32, label="rewards")
    _lib.check(sdlib.sd_op_reward_head(_lib.current_stream(), guarded_input(hid).data_ptr(), L * H, guarded_input(w).data_ptr(),
                                       guarded_input(bias).data_ptr(), mean, std, B, H, r2.data_ptr(), None))
    torch.cuda.synchronize()
    assert torch.equal(r2.cpu(), rewards.cpu())
    check_guards()


# ---- the tiny model end to end ----------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def tiny_dir(tmp_path_factory):
    return U.write_tiny_dir(str(tmp_path_factory.mktemp("image_reward") / "tiny"))


@pytest.fixture(scope="module")
def tiny_model(tiny_dir):
    return IR.HipImageReward.from_pretrained(tiny_dir)


@pytest.fixture(scope="module")
def tiny_ref():
    cfg, sd, tok, images = U.tiny_config(), U.tiny_state_dict(), U.tiny_tokenizer(), U.tiny_images()
    f = O.features(sd, cfg, tok, U.PROMPTS, images)
    return cfg, sd, tok, images, f, O.reward_head(sd, cfg, f)


def _check(f, r, f_ref, r_ref, cfg, sd, what):
    per = ((f.double() - f_ref.double()).norm(dim=-1) / f_ref.double().norm(dim=-1))
    tr = U.tol_r(cfg, sd, f_ref)
    dr = (r.double() - r_ref.double()).abs()
    print(f"{what}: features rel-L2 per sample max {float(per.max()):.3e} (gate {TOL}), "
          f"rewards |err| / tol_r max {float((dr / tr).max()):.3e}")
    assert torch.isfinite(f).all() and (per <= TOL).all(), f"{what}: per-sample feature rel-L2 {per.tolist()}"
    assert (dr <= tr).all(), f"{what}: reward errors {dr.tolist()} vs tol_r {tr.tolist()}"


def test_tiny_model_matches_golden_and_oracle(tiny_model, tiny_ref):
    cfg, sd, tok, images, f_ref, r_ref = tiny_ref
    golden = json.load(open(GOLDEN))
    # the list call groups the interleaved sizes; prompts include [CLS][SEP] only (4) and the truncated one (5)
    f = tiny_model.features(U.PROMPTS, images).cpu()
    r = tiny_model.score(U.PROMPTS, images).cpu()
    _check(f, r, f_ref, r_ref, cfg, sd, "tiny vs oracle")
    _check(f, r, torch.tensor(golden["features"]), torch.tensor(golden["rewards"]), cfg, sd, "tiny vs transformers golden")
    # grouping: every image scored alone gives the same reward as in its group (same plan shape per size: batch 1 vs 2 may
    # pick other GEMM tiles, so the comparison is at the reward tolerance, not bitwise)
    for i in (1, 2, 7):
        ri = tiny_model.score([U.PROMPTS[i]], images[i][None]).cpu()
        assert abs(float(ri[0]) - float(r_ref[i])) <= float(U.tol_r(cfg, sd, f_ref)[i])
    # a tensor batch of one size equals the list call on the same images
    same = [images[0], images[4]]
    rt = tiny_model.score([U.PROMPTS[0], U.PROMPTS[4]], torch.stack(same)).cpu()
    assert torch.equal(rt, tiny_model.score([U.PROMPTS[0], U.PROMPTS[4]], same).cpu())
    with pytest.raises(ValueError, match="prompts"):
        tiny_model.score(["a", "b"], images[:3])


def test_tiny_inference_rank_is_the_oracles(tiny_model, tiny_ref):
    cfg, sd, tok, images, _, _ = tiny_ref
    sel = [images[i] for i in U.RANK_IMAGES]
    ranks, rewards = tiny_model.inference_rank(U.RANK_PROMPT, sel)
    oranks, orewards = O.inference_rank(sd, cfg, tok, U.RANK_PROMPT, sel)
    print(f"ranks {ranks} (oracle {oranks}); rewards {rewards} (oracle {orewards})")
    assert ranks == oranks and sorted(ranks) == [1, 2, 3, 4]
    assert ranks[max(range(4), key=lambda i: rewards[i])] == 1


def test_score_refuses_an_all_masked_prompt(tiny_model, tiny_ref):
    images = tiny_ref[3]
    ids, mask = tiny_model.tokenizer(["a cat"])
    with pytest.raises(_lib.SdHipError, match="no valid key"):
        with torch.cuda.device(tiny_model.device):
            tiny_model._score_batch(images[0][None], ids, torch.zeros_like(mask))


# ---- the v1.0 shape ---------------------------------------------------------------------------------------------------

def test_full_shape_matches_oracle():
    """ViT-L/16 + BERT-base with 12 cross-attending layers, synthetic weights, two images: the only place where 197 keys, 12
    heads and the one-GEMM K|V at N = 18432 meet."""
    cfg = IR.ImageRewardConfig(vocab_size=len(U.synthetic_vocab()))         # (the vocabulary only sizes the embedding table)
    IR.check_image_reward_config(cfg)
    assert cfg.num_hidden_layers * 2 * cfg.hidden_size == 18432 and cfg.image_tokens == 197
    sd = IR.make_synthetic_image_reward_state_dict(cfg, seed=4242)
    tok = IR.BertWordPieceTokenizer({t: i for i, t in enumerate(U.synthetic_vocab())}, max_length=cfg.max_text_len)
    images = [U.seeded_image(240, 300, 31), U.seeded_image(240, 300, 32)]
    prompts = ["a photo of the red cat and the blue hat", U.PROMPTS[5]]
    m = IR.HipImageReward(cfg, sd, tok)
    f = m.features(prompts, torch.stack(images)).cpu()
    r = m.score(prompts, torch.stack(images)).cpu()
    f_ref = O.features(sd, cfg, tok, prompts, images)
    _check(f, r, f_ref, O.reward_head(sd, cfg, f_ref), cfg, sd, "v1.0 shape vs oracle")


# ---- metric and wiring ------------------------------------------------------------------------------------------------

def test_reward_model_win_rate_is_the_oracles(tiny_dir, tiny_ref):
    from sonicdiffusionbayeslab_amd.metrics import RewardModel
    cfg, sd, tok, images, _, _ = tiny_ref
    wins = U.oracle_decisions(cfg, sd, tok, images)
    m = RewardModel("ImageReward-v1.0", model_path=tiny_dir)
    assert m.model is None
    prompts = [U.PROMPTS[p] for _, _, p in U.PAIRS]
    real, gen = [images[r] for r, _, _ in U.PAIRS], [images[g] for _, g, _ in U.PAIRS]
    m.update(real[:4], gen[:4], prompts[:4])
    m.update(real[4:], gen[4:], prompts[4:])
    print(f"win rate {float(m.compute()):.4f}, oracle decisions {wins}")
    assert m.total == len(U.PAIRS) and m.wins == sum(wins) and float(m.compute()) == pytest.approx(sum(wins) / len(wins))
    m.reset()
    assert m.total == 0 and torch.isnan(m.compute())
    m.update(real[:1], gen[:1], prompts[:1])
    assert float(m.compute()) == float(wins[0])
    mean = m.calc_metric(gen, prompts)
    ref = float(O.score(sd, cfg, tok, prompts, gen).double().mean())
    assert abs(mean - ref) <= float(U.tol_r(cfg, sd, O.features(sd, cfg, tok, prompts, gen)).max())


def test_validate_reports_image_reward(tiny_dir, tmp_path, capsys):
    from PIL import Image
    from sonicdiffusionbayeslab_amd.config import _wrap
    from sonicdiffusionbayeslab_amd.experiments.base_experiment import BaseMethod
    from sonicdiffusionbayeslab_amd.weights import UNetConfig
    all_prompts = json.load(open(os.path.join(ROOT, "data", "dataset", "img2annotations_test.json")))
    names = sorted(all_prompts)[:4]
    img_dir = str(tmp_path / "imgs")
    os.makedirs(img_dir)
    for i, n in enumerate(names):
        Image.fromarray(U.seeded_image(64, 64, 50 + i).permute(1, 2, 0).numpy(), "RGB").save(os.path.join(img_dir, n))
    pf = tmp_path / "prompts.json"
    pf.write_text(json.dumps({k: all_prompts[k] for k in names}))
    decoded = []

    class _Stub:            # a pipeline that "decodes" seeded images in [0, 1]
        weights_source, num_timesteps = "stub", 2

        def __init__(self):
            self.unet_config = UNetConfig(sample_size=8)
            self.scheduler = type("S", (), {"config": {}})()

        def to(self, device):
            return self

        def __call__(self, prompts, generator=None, output_type="pt", **kw):
            imgs = torch.rand((len(prompts), 3, 64, 64), generator=generator)
            decoded.extend(imgs)
            return type("O", (), {"images": imgs})(), 0.1, []

    class M(BaseMethod):
        def setup_model(self):
            self.model = _Stub()

        def setup_scheduler(self, **kw):
            pass

        def run_experiment(self):
            self.sweep([2], lambda n: {"num_inference_steps": n}, lambda n: f"steps {n}")

    base = {"experiment_name": "stub", "experiment": {"method": "stub", "seed": 29},
            "dataset": {"img_dataset": img_dir, "prompts": str(pf), "image_size": 64},
            "inference": {"batch_size": 4, "batch_count": 1}}
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "SD_DIST_FORCE_INIT"):
        os.environ.pop(k, None)
    m = M(_wrap(dict(base, quality_metrics={"image_reward": {"model_name": "ImageReward-v1.0", "model_path": tiny_dir}})))
    assert m.image_reward_metric is not None and m.image_reward_metric.model is None
    m.run_experiment()
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    scorer = m.image_reward_metric.model
    gen = (torch.stack(decoded) * 255).to(torch.uint8)
    real = (m.load_images(m.last_image_files) * 255).to(torch.uint8)
    want = float((scorer.score(m.last_prompts, real) <= scorer.score(m.last_prompts, gen)).float().mean())
    print(f"validate image_reward: {line['image_reward']}, the scorer alone {want}")
    assert line["images"] == 4 and line["image_reward_model"] == tiny_dir and line["image_reward"] == want
    assert m.metric_dict["image_reward"] == [line["image_reward"]]
    # without the key: the fields a run had before, nothing else
    k = M(_wrap(base))
    assert k.image_reward_metric is None and k.image_reward_source == "not configured"
    k.run_experiment()
    line2 = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert "image_reward" not in line2 and "image_reward_model" not in line2 and "image_reward" not in k.metric_dict
    assert set(line) - set(line2) == {"image_reward", "image_reward_model"}
    # the key without a local directory: null and the reason
    q = M(_wrap(dict(base, quality_metrics={"image_reward": {"model_name": "ImageReward-v1.0"}})))
    q.run_experiment()
    line3 = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert line3["image_reward"] is None and "not computable offline" in line3["image_reward_model"]
