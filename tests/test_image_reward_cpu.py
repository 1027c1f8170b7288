"""ImageReward, host side: the WordPiece tokenizer against recorded BertTokenizer ids, the fp32 oracle against recorded
transformers BLIP features and rewards (tests/golden/make_image_reward_golden.py), the folded reward head, the name table and
config errors, the metric's counting with a stand-in scorer, and setup_metrics' reporting.

The gap condition behind the GPU win-rate and rank checks is enforced here: with tol_r = TOL ||f_ref|| ||w_fold|| / std per
sample (what a feature error of TOL rel-L2 can move a reward by, Cauchy-Schwarz on the folded head), every real / generated
pair of tests/image_reward_util.PAIRS and every neighbouring pair of the ranked images has an oracle reward gap above
2 tol_r, so no decision can flip within the feature tolerance."""
import json
import os

import pytest
import torch

from sonicdiffusionbayeslab_amd import _lib
from sonicdiffusionbayeslab_amd import image_reward as IR
from tests import image_reward_oracle as O
from tests import image_reward_util as U
from tests.util import rel_l2

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "image_reward_golden.json")


@pytest.fixture(scope="module")
def golden():
    return json.load(open(GOLDEN))


@pytest.fixture(scope="module")
def tiny():
    return U.tiny_config(), U.tiny_state_dict(), U.tiny_tokenizer(), U.tiny_images()


@pytest.fixture(scope="module")
def oracle_feats(tiny):
    cfg, sd, tok, images = tiny
    return O.features(sd, cfg, tok, U.PROMPTS, images)


def test_tokenizer_matches_bert_tokenizer_ids(golden, tiny):
    tok = tiny[2]
    assert golden["prompts"] == U.PROMPTS
    ids, mask = tok(U.PROMPTS)
    assert ids.tolist() == golden["input_ids"] and mask.tolist() == golden["attention_mask"]
    v = tok.vocab
    # case and accents fold onto the plain words; punctuation splits; an unknown word is one [UNK]
    assert tok.encode("A Photo of THE Cat") == [v["[CLS]"], v["a"], v["photo"], v["of"], v["the"], v["cat"], v["[SEP]"]]
    assert tok.encode("naïve café") == [v["[CLS]"], v["naive"], v["cafe"], v["[SEP]"]]
    assert tok.encode("cat's") == [v["[CLS]"], v["cat"], v["'"], v["s"], v["[SEP]"]]
    assert tok.encode("a quartz dog") == [v["[CLS]"], v["a"], v["[UNK]"], v["dog"], v["[SEP]"]]
    assert tok.encode("dogs") == [v["[CLS]"], v["dog"], v["##s"], v["[SEP]"]]
    assert tok.encode("a" * 101) == [v["[CLS]"], v["[UNK]"], v["[SEP]"]]
    # the empty prompt is [CLS] [SEP]; a long one is cut at 35 and keeps its [SEP]
    assert ids[4, :3].tolist() == [v["[CLS]"], v["[SEP]"], 0] and int(mask[4].sum()) == 2
    assert int(mask[5].sum()) == 35 and ids[5, 34] == v["[SEP]"] and ids[5, 0] == v["[CLS]"]


def test_oracle_matches_transformers_golden(golden, tiny, oracle_feats):
    cfg, sd, _, _ = tiny
    gf, gr = torch.tensor(golden["features"]), torch.tensor(golden["rewards"])
    ef = rel_l2(oracle_feats, gf)
    rw = O.reward_head(sd, cfg, oracle_feats)
    er = rel_l2(rw, gr)
    print(f"oracle vs transformers {golden['transformers']}: features rel-L2 {ef:.3e}, rewards rel-L2 {er:.3e}")
    assert ef <= 1e-5 and er <= 1e-5


def test_padded_ids_do_not_reach_the_reward(tiny, oracle_feats):
    cfg, sd, tok, images = tiny
    ids, mask = tok(U.PROMPTS)
    g = torch.Generator().manual_seed(3)
    junk = torch.randint(1, cfg.vocab_size, ids.shape, generator=g, dtype=torch.int32)
    ids2 = torch.where(mask.bool(), ids, junk)
    assert not torch.equal(ids, ids2)
    f2 = O.features_from_ids(sd, cfg, ids2, mask, images)
    d = float((O.reward_head(sd, cfg, f2) - O.reward_head(sd, cfg, oracle_feats)).abs().max())
    print(f"reward change under junk padded ids: {d:.3e}")
    assert d <= 1e-5


def test_folded_head_equals_the_chain(tiny):
    _, sd, _, _ = tiny
    w, b = IR.fold_reward_head(sd)
    g = torch.Generator().manual_seed(5)
    x = torch.randn(16, w.numel(), generator=g, dtype=torch.float64) * 3
    y = x
    for k in IR.HEAD_LAYERS:
        y = y @ sd[f"mlp.layers.{k}.weight"].double().t() + sd[f"mlp.layers.{k}.bias"].double()
    err = (x @ w + b - y[:, 0]).abs()
    mag = (x.abs() @ w.abs()) + abs(b)
    print(f"folded head vs chain: worst err / (sum |w x| + |b|) = {float((err / mag).max()):.3e}")
    assert (err <= 1e-10 * mag).all()


def test_name_table_and_shape_errors_name_the_key(tiny):
    cfg, sd, _, _ = tiny
    table = IR.image_reward_name_table(cfg)
    assert len(table) == len(sd) and {t[0] for t in table} == set(sd)
    assert [t[1] for t in table] == [n for n, _ in IR.image_reward_param_shapes(cfg)]
    m = IR.map_image_reward_state_dict(cfg, sd)
    assert m["visual_encoder.cls_token"].shape == (192,) and m["visual_encoder.pos_embed"].shape == (17, 192)
    key = "blip.text_encoder.encoder.layer.1.crossattention.self.key.weight"
    assert sd[key].shape == (128, 192)
    with pytest.raises(KeyError, match="crossattention.self.key.weight"):
        IR.map_image_reward_state_dict(cfg, {k: v for k, v in sd.items() if k != key})
    with pytest.raises(ValueError, match="blip.visual_encoder.pos_embed"):
        IR.map_image_reward_state_dict(cfg, dict(sd, **{"blip.visual_encoder.pos_embed": torch.zeros(1, 16, 192)}))
    with pytest.raises(ValueError, match="mlp.layers.7.weight"):
        IR.map_image_reward_state_dict(cfg, dict(sd, **{"mlp.layers.7.weight": torch.zeros(2, 16)}))


@pytest.mark.parametrize("field,value", [
    ("vision_num_attention_heads", 2), ("num_attention_heads", 4), ("vision_hidden_size", 1600), ("hidden_size", 100),
    ("image_size", 320), ("max_text_len", 65), ("hidden_act", "relu"), ("position_embedding_type", "relative_key"),
    ("intermediate_size", 100), ("vision_intermediate_size", 0), ("patch_size", 24)])
def test_refused_config_fields_are_named(field, value):
    import dataclasses
    cfg = dataclasses.replace(U.tiny_config(), **{field: value})
    if field == "vision_hidden_size":
        cfg = dataclasses.replace(cfg, vision_num_attention_heads=25)
    with pytest.raises(ValueError, match=field):
        IR.check_image_reward_config(cfg)
    IR.check_image_reward_config(U.tiny_config())
    IR.check_image_reward_config(IR.ImageRewardConfig())           # the v1.0 shape itself


def test_read_dir_and_refusals(tmp_path):
    d = U.write_tiny_dir(str(tmp_path / "ir"))
    cfg, weights, vocab = IR.read_image_reward_dir(d)
    assert cfg == U.tiny_config() and weights.endswith("ImageReward.safetensors") and vocab.endswith("vocab.txt")
    assert set(IR.load_image_reward_weights(weights)) == set(U.tiny_state_dict())
    med = json.load(open(os.path.join(d, "med_config.json")))
    json.dump(dict(med, hidden_act="relu"), open(os.path.join(d, "med_config.json"), "w"))
    with pytest.raises(ValueError, match="hidden_act"):
        IR.read_image_reward_dir(d)
    os.remove(os.path.join(d, "vocab.txt"))
    with pytest.raises(FileNotFoundError, match="vocab.txt"):
        IR.read_image_reward_dir(d)


def test_reward_model_needs_a_local_directory(tmp_path):
    from sonicdiffusionbayeslab_amd.metrics import RewardModel
    from sonicdiffusionbayeslab_amd.registry import metrics_registry
    assert metrics_registry["image_reward"] is RewardModel
    for kw in ({}, {"model_path": "/no/such/dir"}, {"model_path": None, "device": "cuda"}):
        with pytest.raises(FileNotFoundError, match="network fetch.*pass a local directory"):
            RewardModel("ImageReward-v1.0", **kw)
    m = RewardModel("ImageReward-v1.0", model_path=U.write_tiny_dir(str(tmp_path / "ir")))
    assert m.model is None and m.wins == 0 and m.total == 0           # nothing is built before the first update


def test_win_rate_counting_with_a_stand_in_scorer(tmp_path):
    from sonicdiffusionbayeslab_amd.metrics import RewardModel
    m = RewardModel(model_path=U.write_tiny_dir(str(tmp_path / "ir")))

    class Stand:                  # the reward of an image is its first pixel
        def score(self, prompts, images):
            assert len(prompts) == len(images)
            return torch.stack([im.flatten()[0].float() for im in images])

    m.model = Stand()
    img = lambda v: torch.full((3, 4, 4), v, dtype=torch.uint8)
    assert torch.isnan(m.compute())
    m.update([img(1), img(5), img(7)], [img(2), img(5), img(3)], ["a", "b", "c"])      # win, tie (a win), loss
    assert (m.wins, m.total) == (2, 3) and float(m.compute()) == pytest.approx(2 / 3)
    m.update([img(9)], [img(0)], ["d"])
    assert (m.wins, m.total) == (2, 4) and float(m.compute()) == 0.5
    m.reset()
    assert (m.wins, m.total) == (0, 0) and torch.isnan(m.compute())
    assert m.calc_metric([img(1), img(2), img(6)], ["a", "b", "c"]) == 3.0


def test_setup_metrics_reports_the_three_sources(tmp_path):
    from sonicdiffusionbayeslab_amd.experiments.base_experiment import BaseMethod

    class Cfg(dict):
        __getattr__ = dict.get

    class Probe(BaseMethod):
        def __init__(self, cfg):
            self.config, self.device = cfg, "cpu"

        def run_experiment(self):
            pass

    p = Probe(Cfg(quality_metrics=Cfg(clip_score=Cfg(model_name_or_path="openai/clip-vit-base-patch16"))))
    p.setup_metrics()
    assert p.image_reward_metric is None and p.image_reward_source == "not configured" and not p.image_reward_configured
    assert p.image_reward([torch.zeros(3, 8, 8)], ["x"], ["a.png"]) is None
    q = Probe(Cfg(quality_metrics=Cfg(image_reward=Cfg(model_name="ImageReward-v1.0"))))
    q.setup_metrics()
    assert q.image_reward_metric is None and q.image_reward_configured
    assert "not computable offline" in q.image_reward_source and "ImageReward-v1.0" in q.image_reward_source
    d = U.write_tiny_dir(str(tmp_path / "ir"))
    r = Probe(Cfg(quality_metrics=Cfg(image_reward=Cfg(model_name="ImageReward-v1.0", model_path=d))))
    r.setup_metrics()
    assert r.image_reward_metric is not None and r.image_reward_source == d and r.image_reward_metric.model is None


def test_new_symbols_are_exported_and_declared():
    names = ["sd_image_reward_create", "sd_image_reward_workspace_bytes", "sd_image_reward_score", "sd_op_bert_attention",
             "sd_op_reward_head"]
    lib = _lib.load()
    for n in names:
        assert n in _lib._SIGS and n in _lib.declared_symbols(), n
        assert getattr(lib, n) is not None


def test_library_enumerates_the_name_table_and_refuses_by_name():
    """sd_image_reward_create is host-only: the handle's parameter list is the Python table, and each limit is named."""
    import ctypes as C
    lib = _lib.load()
    cfg = U.tiny_config()

    def make(c):
        return _lib.SdImageRewardConfig(
            c.vision_hidden_size, c.vision_num_hidden_layers, c.vision_num_attention_heads, c.vision_intermediate_size,
            c.image_size, c.patch_size, c.vision_layer_norm_eps, c.vocab_size, c.hidden_size, c.num_hidden_layers,
            c.num_attention_heads, c.intermediate_size, c.max_position_embeddings, c.layer_norm_eps, 1, 1, c.max_text_len,
            c.reward_mean, c.reward_std)

    h = C.c_void_p()
    assert lib.sd_image_reward_create(C.byref(make(cfg)), C.byref(h)) == 0
    try:
        got = []
        name, shape, nd = C.create_string_buffer(256), (C.c_longlong * 4)(), C.c_int()
        for i in range(lib.sd_unet_num_params(h)):
            assert lib.sd_unet_param_info(h, i, name, 256, shape, C.byref(nd)) == 0
            got.append((name.value.decode(), tuple(shape[k] for k in range(nd.value))))
        assert got == IR.image_reward_param_shapes(cfg)
    finally:
        lib.sd_unet_destroy(h)
    import dataclasses
    for field, value, word in (("max_text_len", 65, "max_text_len"), ("num_attention_heads", 4, "num_heads"),
                               ("image_size", 320, "image tokens"), ("hidden_size", 1600, "hidden_size")):
        bad = make(dataclasses.replace(cfg, **{field: value}))
        h2 = C.c_void_p()
        assert lib.sd_image_reward_create(C.byref(bad), C.byref(h2)) != 0
        assert word in lib.sd_last_error().decode(), lib.sd_last_error()
    for slot, word in ((14, "hidden_act"), (15, "position_embedding_absolute")):
        bad = make(cfg)
        setattr(bad, _lib.SdImageRewardConfig._fields_[slot][0], 0)
        assert lib.sd_image_reward_create(C.byref(bad), C.byref(C.c_void_p())) != 0 and word in lib.sd_last_error().decode()


def test_gap_condition_of_the_gpu_decisions(tiny):
    """Every win-rate pair and every neighbouring pair of the ranked images is decided by more than 2 tol_r."""
    cfg, sd, tok, images = tiny
    for real, gen, p in U.PAIRS:
        f = O.features(sd, cfg, tok, [U.PROMPTS[p]] * 2, [images[real], images[gen]])
        r = O.reward_head(sd, cfg, f).double()
        t = U.tol_r(cfg, sd, f)
        gap = float((r[0] - r[1]).abs())
        print(f"pair real {real} gen {gen} prompt {p}: rewards {r.tolist()}, gap {gap:.3f}, 2 tol_r {2 * float(t.max()):.3f}")
        assert gap > 2 * float(t.max())
    sel = [images[i] for i in U.RANK_IMAGES]
    f = O.features(sd, cfg, tok, U.RANK_PROMPT, sel)
    r = O.reward_head(sd, cfg, f).double()
    t = float(U.tol_r(cfg, sd, f).max())
    s = torch.sort(r).values
    print(f"ranked rewards {r.tolist()}, smallest neighbour gap {float((s[1:] - s[:-1]).min()):.3f}, 2 tol_r {2 * t:.3f}")
    assert float((s[1:] - s[:-1]).min()) > 2 * t
    wins = [bool(x) for x in U.oracle_decisions(cfg, sd, tok, images)]
    assert 0 < sum(wins) < len(wins)                                  # the win rate is neither 0 nor 1: both outcomes are tested
