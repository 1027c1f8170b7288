"""Inpainting without a GPU: the new exports, every argument check before any GPU work, the strength default that switches
with ``mask_image``, ``read_unet_config`` for 4 / 9 / other input channels, the mask helpers, the oracle's mask processing,
the 9-channel handle's parameter table and the harness key ``experiment_params.inpaint_box``."""
import ctypes as C
import json
import os

import pytest
import torch

from sonicdiffusionbayeslab_amd import _lib

NEW_SYMBOLS = ["sd_inpaint_prepare", "sd_sched_step_inpaint", "sd_unet_set_inpaint_cond_hw", "sd_op_conv_in_cond"]


def test_inpaint_symbols_are_exported_and_the_abi_version_stays():
    lib = _lib.load()
    for n in NEW_SYMBOLS:
        assert hasattr(lib, n), n
        assert n in _lib._SIGS and n in _lib.declared_symbols(), n
    assert lib.sd_abi_version() == 3
    # the entry points that existed keep their signatures
    assert len(_lib._SIGS["sd_sched_step"][1]) == 14 and len(_lib._SIGS["sd_sched_step_rescaled"][1]) == 16
    assert len(_lib._SIGS["sd_op_conv_in"][1]) == 11


def _model(sample_size=64, in_channels=4):
    from sonicdiffusionbayeslab_amd.models import StableDiffusionModel
    from sonicdiffusionbayeslab_amd.registry import schedulers_registry
    from sonicdiffusionbayeslab_amd.weights import UNetConfig
    m = StableDiffusionModel(unet_config=UNetConfig(sample_size=sample_size, in_channels=in_channels), state_dict={})
    m.scheduler = schedulers_registry["ddim_scheduler"].from_config(m.scheduler.config)
    return m


def _no_gpu(model, monkeypatch):
    def boom(*a, **k):
        raise AssertionError("the arguments must be checked before the UNet is built")
    monkeypatch.setattr(model, "_ensure_unet", boom)


def test_mask_argument_errors_come_before_any_gpu_work(monkeypatch):
    from sonicdiffusionbayeslab_amd.registry import schedulers_registry
    model = _model()
    _no_gpu(model, monkeypatch)
    pe = torch.zeros(1, 77, 768)
    img = torch.rand(1, 3, 512, 768)
    mask = torch.zeros(1, 1, 512, 768)
    call = lambda **kw: model(**{**dict(prompt_embeds=pe, negative_prompt_embeds=pe, image=img, mask_image=mask,
                                        num_inference_steps=10, output_type="latent"), **kw})
    with pytest.raises(ValueError, match="does not match the image size"):
        call(mask_image=torch.zeros(1, 1, 512, 512))
    with pytest.raises(ValueError, match="does not match the image size"):
        call(mask_image=torch.zeros(1, 768, 512))
    with pytest.raises(ValueError, match="mask_image batch"):
        call(mask_image=torch.zeros(2, 1, 512, 768))
    with pytest.raises(ValueError, match="mask_image without image"):
        call(image=None)
    with pytest.raises(ValueError, match="float tensor"):
        call(mask_image=torch.zeros(1, 1, 512, 768, dtype=torch.uint8))
    with pytest.raises(ValueError, match="float tensor"):
        call(mask_image=torch.zeros(1, 3, 512, 768))
    with pytest.raises(NotImplementedError, match="padding_mask_crop"):
        call(padding_mask_crop=32)
    with pytest.raises(NotImplementedError, match="padding_mask_crop"):
        model(prompt_embeds=pe, negative_prompt_embeds=pe, padding_mask_crop=32, num_inference_steps=10)
    # latents= is the forward noise, at strength 1.0 only
    lat = torch.zeros(1, 4, 64, 96)
    with pytest.raises(ValueError, match="only at strength == 1.0"):
        call(latents=lat, strength=0.5)
    with pytest.raises(ValueError, match="only at strength == 1.0"):
        call(latents=lat, strength=0.99)
    with pytest.raises(ValueError, match="do not match the image"):
        call(latents=torch.zeros(1, 4, 64, 64))
    with pytest.raises(AssertionError, match="before the UNet is built"):
        call(latents=lat)                                   # strength defaults to 1.0 with a mask
    with pytest.raises(AssertionError, match="before the UNet is built"):
        call(latents=lat, strength=1.0)
    # the checks of image-to-image still hold
    with pytest.raises(ValueError, match="strength"):
        call(strength=1.5)
    with pytest.raises(ValueError, match="at least one"):
        call(strength=0.05)
    with pytest.raises(ValueError, match="sample_mode"):
        call(sample_mode="mean")
    with pytest.raises(ValueError, match="disagrees"):
        call(height=512, width=512)
    # [B, H, W] masks and PIL masks are accepted
    with pytest.raises(AssertionError, match="before the UNet is built"):
        call(mask_image=torch.zeros(1, 512, 768))
    from PIL import Image
    with pytest.raises(AssertionError, match="before the UNet is built"):
        model(["a"], image=[Image.new("RGB", (768, 512))], mask_image=[Image.new("L", (768, 512), 255)], num_inference_steps=10)
    with pytest.raises(ValueError, match="does not match the image size"):
        model(["a"], image=[Image.new("RGB", (768, 512))], mask_image=[Image.new("L", (512, 512), 255)], num_inference_steps=10)
    # PNDM (the checkpoint's scheduler) is refused by name
    from sonicdiffusionbayeslab_amd.schedulers import PNDMConfigStub
    model.scheduler = schedulers_registry["pndm_scheduler"].from_config(PNDMConfigStub().config)
    with pytest.raises(NotImplementedError, match="PNDMScheduler"):
        call()


def test_strength_default_switches_with_the_mask(monkeypatch):
    """With ``mask_image`` the default is 1.0 (every step runs, ``latents=`` allowed); without it 0.8; explicit values win."""
    model = _model()
    seen = {}

    def inpaint(prompt, image, mask_image, strength, *a):
        seen["inpaint"] = strength
        return None, 0.0, []

    def img2img(prompt, image, strength, *a):
        seen["img2img"] = strength
        return None, 0.0, []
    monkeypatch.setattr(model, "_call_inpaint", inpaint)
    monkeypatch.setattr(model, "_call_img2img", img2img)
    pe = torch.zeros(1, 77, 768)
    img, mask = torch.rand(1, 3, 512, 512), torch.zeros(1, 1, 512, 512)
    model(prompt_embeds=pe, image=img, mask_image=mask)
    assert seen.pop("inpaint") == 1.0
    model(prompt_embeds=pe, image=img, mask_image=mask, strength=0.8)
    assert seen.pop("inpaint") == 0.8
    model(prompt_embeds=pe, image=img)
    assert seen.pop("img2img") == 0.8
    model(prompt_embeds=pe, image=img, strength=1.0)
    assert seen.pop("img2img") == 1.0
    assert not seen


def test_nine_channel_unet_runs_only_with_a_mask(monkeypatch):
    model = _model(in_channels=9)
    _no_gpu(model, monkeypatch)
    pe = torch.zeros(1, 77, 768)
    with pytest.raises(ValueError, match="9 input channels.*text-to-image"):
        model(prompt_embeds=pe, negative_prompt_embeds=pe, num_inference_steps=4, output_type="latent")
    with pytest.raises(ValueError, match="9 input channels.*image-to-image"):
        model(prompt_embeds=pe, negative_prompt_embeds=pe, image=torch.rand(1, 3, 512, 512), num_inference_steps=4,
              output_type="latent")
    with pytest.raises(AssertionError, match="before the UNet is built"):
        model(prompt_embeds=pe, negative_prompt_embeds=pe, image=torch.rand(1, 3, 512, 512),
              mask_image=torch.ones(1, 1, 512, 512), num_inference_steps=4, output_type="latent")


def test_variant_pipelines_refuse_a_mask(monkeypatch):
    from sonicdiffusionbayeslab_amd import models as M
    from sonicdiffusionbayeslab_amd.weights import UNetConfig
    pe = torch.zeros(1, 77, 768)
    img, mask = torch.rand(1, 3, 512, 512), torch.ones(1, 1, 512, 512)
    for cls, kw in [(M.StableDiffusionModelSkipTimesteps, dict(num_inference_steps=2, skip_timesteps=[])),
                    (M.StableDiffusionModelInterlivingSchedulers, dict(num_inference_steps=2, interliving_steps=[])),
                    (M.StableDiffusionModelTwoSchedulers, dict(num_inference_steps_first=2))]:
        model = cls(unet_config=UNetConfig(sample_size=64), state_dict={})
        model.scheduler_first = model.scheduler_second = model.scheduler_main = model.scheduler_inter = model.scheduler
        _no_gpu(model, monkeypatch)
        with pytest.raises(NotImplementedError, match="mask_image"):
            model(prompt_embeds=pe, negative_prompt_embeds=pe, image=img, mask_image=mask, output_type="latent", **kw)
        with pytest.raises(NotImplementedError, match="mask_image"):
            model(prompt_embeds=pe, negative_prompt_embeds=pe, mask_image=mask, output_type="latent", **kw)


def test_pndm_step_refuses_the_blend_by_name():
    from sonicdiffusionbayeslab_amd.registry import schedulers_registry
    from sonicdiffusionbayeslab_amd.schedulers import PNDMConfigStub
    s = schedulers_registry["pndm_scheduler"].from_config(PNDMConfigStub().config)
    s.set_timesteps(4)
    x = torch.zeros(1, 4, 8, 8)
    with pytest.raises(NotImplementedError, match="PNDMScheduler"):
        s.step_fused(x, 1.0, x, s._timesteps_list[0], cfg=False, inpaint=(x, x, torch.ones(1, 1, 8, 8), None))


def test_blend_coefficients_come_from_add_noise_coefs():
    """(a, s) of the launch: ``_add_noise_coefs`` of the next timestep, (1, 0) after the last step; shapes are checked."""
    import math
    from sonicdiffusionbayeslab_amd.registry import schedulers_registry
    from sonicdiffusionbayeslab_amd.schedulers import PNDMConfigStub
    s = schedulers_registry["ddim_scheduler"].from_config(PNDMConfigStub().config)
    s.set_timesteps(10)
    s._prep = lambda t: t                                # (host tensors: only the bookkeeping is under test)
    x, m = torch.zeros(2, 4, 8, 8), torch.ones(2, 1, 8, 8)
    t = s._timesteps_list[3]
    init, noise, mask, a, sg = s._blend((x, x, m, t), x)
    ac = float(s.alphas_cumprod[t])
    assert (a, sg) == (math.sqrt(ac), math.sqrt(1.0 - ac)) and mask is m
    assert s._blend((x, x, m, None), x)[3:] == (1.0, 0.0)
    assert s._blend(None, x) is None
    with pytest.raises(ValueError, match="mask"):
        s._blend((x, x, torch.ones(2, 4, 8, 8), t), x)
    with pytest.raises(ValueError, match="mask"):
        s._blend((x, x, torch.ones(1, 1, 8, 8), t), x)
    with pytest.raises(ValueError, match="do not match the sample"):
        s._blend((torch.zeros(2, 4, 8, 4), x, m, t), x)


def _unet_json(**kw):
    return {"sample_size": 64, "in_channels": 4, "out_channels": 4, "block_out_channels": [320, 640, 1280, 1280],
            "attention_head_dim": 8, "cross_attention_dim": 768, **kw}


def test_read_unet_config_passes_4_and_9_input_channels_and_refuses_others(tmp_path):
    from sonicdiffusionbayeslab_amd.weights import load_unet_config, param_shapes, read_unet_config
    assert read_unet_config(_unet_json()).in_channels == 4
    c9 = read_unet_config(_unet_json(in_channels=9))
    assert c9.in_channels == 9 and c9.out_channels == 4
    assert dict(param_shapes(c9))["conv_in.weight"] == (320, 9, 3, 3)
    for bad in (5, 8, 3, "9", True):
        with pytest.raises(NotImplementedError, match="in_channels"):
            read_unet_config(_unet_json(in_channels=bad))
    d = tmp_path / "unet"
    d.mkdir()
    (d / "config.json").write_text(json.dumps(_unet_json(in_channels=9)))
    assert load_unet_config(str(tmp_path)).in_channels == 9
    (d / "config.json").write_text(json.dumps(_unet_json(in_channels=5)))
    with pytest.raises(NotImplementedError, match="in_channels=5"):
        load_unet_config(str(tmp_path))


def test_library_accepts_4_and_9_input_channels_and_names_both():
    from sonicdiffusionbayeslab_amd.unet import _c_config
    from sonicdiffusionbayeslab_amd.weights import UNetConfig, param_shapes
    lib = _lib.load()
    for cin in (4, 9):
        cfg = UNetConfig(sample_size=16, in_channels=cin)
        h = C.c_void_p()
        _lib.check(lib.sd_unet_create(C.byref(_c_config(cfg)), C.byref(h)))
        try:
            name, shape, nd = C.create_string_buffer(256), (C.c_longlong * 4)(), C.c_int()
            got = {}
            for i in range(lib.sd_unet_num_params(h)):
                _lib.check(lib.sd_unet_param_info(h, i, name, 256, shape, C.byref(nd)))
                got[name.value.decode()] = tuple(shape[k] for k in range(nd.value))
            assert got["conv_in.weight"] == (320, cin, 3, 3)
            assert got == dict(param_shapes(cfg))
            if cin == 4:            # a 4-channel handle refuses the condition, by name, before touching the device
                assert lib.sd_unet_set_inpaint_cond_hw(h, None, 16, 16, 1, 16, 16) != 0
                assert b"in_channels = 4" in lib.sd_last_error()
        finally:
            lib.sd_unet_destroy(h)
    h = C.c_void_p()
    assert lib.sd_unet_create(C.byref(_c_config(UNetConfig(sample_size=16, in_channels=5))), C.byref(h)) != 0
    msg = lib.sd_last_error().decode()
    assert "in_channels 5" in msg and "4" in msg and "9" in msg


def test_launchers_check_their_arguments_before_launching():
    """Bounds of the new entry points, refused on the host (no device is touched: every call fails in SD_REQUIRE)."""
    lib = _lib.load()
    coef = (C.c_float * 10)()
    p = 256                                                   # any non-null, aligned address: never dereferenced
    for h, w in ((12, 16), (16, 12), (0, 16)):
        assert lib.sd_inpaint_prepare(None, p, p, p, p, 1, h, w) != 0
        assert b"multiples of 8" in lib.sd_last_error()
    assert lib.sd_inpaint_prepare(None, p, None, p, p, 1, 16, 16) != 0
    # hw % 4, n_per_sample % hw, n % n_per_sample, and the noise operand where s != 0
    for n, nps, hw in ((4 * 6, 6 * 4, 6), (4 * 64, 100, 16), (4 * 64 + 64, 4 * 64, 64)):
        assert lib.sd_sched_step_inpaint(None, p, 0, 1.0, p, None, None, None, None, p, None, None, coef, n, None, nps, p, p, p,
                                         1.0, 0.5, hw) != 0, (n, nps, hw)
    assert lib.sd_sched_step_inpaint(None, p, 0, 1.0, p, None, None, None, None, p, None, None, coef, 256, None, 256, p, None, p,
                                     0.5, 0.5, 64) != 0
    assert b"blend_noise" in lib.sd_last_error()
    assert lib.sd_sched_step_inpaint(None, p, 0, 1.0, p, None, None, None, None, p, None, None, coef, 256, None, 256, p, p, None,
                                     0.5, 0.5, 64) != 0
    # conv_in_cond: batch must be a multiple of both source batches
    assert lib.sd_op_conv_in_cond(None, p, 2, p, 3, p, p, p, 4, 8, 8, 64) != 0
    assert lib.sd_op_conv_in_cond(None, p, 2, p, 2, p, p, p, 4, 8, 8, 2048) != 0


def test_mask_tensor_forms():
    from PIL import Image
    from sonicdiffusionbayeslab_amd.models import StableDiffusionModel as M
    t = torch.rand(2, 16, 24)
    assert torch.equal(M._mask_tensor(t), t[:, None]) and M._mask_tensor(t[:, None]).shape == (2, 1, 16, 24)
    a = Image.new("L", (4, 2), 255)
    b = Image.new("RGB", (4, 2), (0, 0, 0))
    m = M._mask_tensor([a, b])
    assert m.shape == (2, 1, 2, 4) and m.dtype == torch.float32
    assert torch.all(m[0] == 1.0) and torch.all(m[1] == 0.0)
    assert M._mask_tensor([Image.new("L", (2, 2), 128)])[0, 0, 0, 0] == torch.tensor(128.0) / 255.0        # (/ 255 in fp32)
    with pytest.raises(ValueError, match="one size"):
        M._mask_tensor([a, Image.new("L", (2, 2))])
    with pytest.raises(ValueError, match="mask_image must be"):
        M._mask_tensor("mask.png")


def test_oracle_mask_processing_is_upstreams():
    """Binarise at 0.5 in pixel space; masked image = (2 img - 1) (m < 0.5) in the [-1, 1] domain; latent mask = nearest
    resize (F.interpolate's default mode) of the binarised mask."""
    import torch.nn.functional as F
    from tests.inpaint_oracle import prepare_mask
    g = torch.Generator().manual_seed(5)
    img = torch.rand(2, 3, 24, 40, generator=g)
    m = torch.rand(2, 1, 24, 40, generator=g)
    below = float(torch.nextafter(torch.tensor(0.5), torch.tensor(0.0)))
    m[0, 0, 0, :4] = torch.tensor([0.5, below, 0.0, 1.0])
    masked, lmask = prepare_mask(img, m)
    binm = (m >= 0.5).float()
    assert torch.equal(2.0 * masked - 1.0, (2.0 * img - 1.0) * (binm < 0.5))
    assert torch.equal(lmask, F.interpolate(binm, size=(3, 5)))
    assert lmask[0, 0, 0, 0] == 1.0 and masked[0, 0, 0, 0] == 0.5 and masked[0, 0, 0, 1] == img[0, 0, 0, 1]


# ---------------------------------------------------------------------------------------------------
# harness: experiment_params.inpaint_box
# ---------------------------------------------------------------------------------------------------
def test_inpaint_box_is_validated():
    from sonicdiffusionbayeslab_amd.experiments.base_experiment import BaseMethod as B
    assert B.parse_inpaint_box(None, 128) is None
    assert B.parse_inpaint_box([8, 16, 64, 128], 128) == (8, 16, 64, 128)
    assert B.parse_inpaint_box((0, 0, 128, 128), 128) == (0, 0, 128, 128)
    for bad in ([8, 16, 64], [8, 16, 64, 130], [8, 16, 64, 136], [4, 16, 64, 128], [64, 16, 64, 128], [8, 64, 64, 32],
                [-8, 0, 64, 64], [8.0, 16, 64, 128], "8,16,64,128", [True, 16, 64, 128], 8):
        with pytest.raises(ValueError, match="inpaint_box"):
            B.parse_inpaint_box(bad, 128)


class _StubOut:
    def __init__(self, images):
        self.images = images


class _StubPipeline:
    weights_source = "stub"
    num_timesteps = 3

    def __init__(self):
        from sonicdiffusionbayeslab_amd.schedulers import SchedulerConfig
        from sonicdiffusionbayeslab_amd.weights import UNetConfig
        self.unet_config = UNetConfig(sample_size=8)
        self.scheduler = type("S", (), {})()
        self.scheduler.config = SchedulerConfig()
        self.calls = []

    def to(self, device):
        return self

    def __call__(self, prompts, **kw):
        self.calls.append(kw)
        return _StubOut(torch.zeros(len(prompts), 4, 8, 8)), 0.25, []


def _harness(tmp, params, img_dir=None):
    from PIL import Image
    from sonicdiffusionbayeslab_amd.config import _wrap
    from sonicdiffusionbayeslab_amd.experiments.base_experiment import BaseMethod
    d = os.path.join(tmp, "img")
    os.makedirs(d, exist_ok=True)
    prompts = {}
    for i in range(3):
        Image.new("RGB", (80, 72), (40 * i, 9, 7)).save(os.path.join(d, f"im{i}.png"))
        prompts[f"im{i}.png"] = f"prompt {i}"
    with open(os.path.join(tmp, "prompts.json"), "w") as f:
        json.dump(prompts, f)

    class M(BaseMethod):
        def setup_model(self):
            self.model = _StubPipeline()

        def setup_scheduler(self, **kw):
            pass

        def run_experiment(self):
            pass

    conf = {"experiment_name": "stub", "experiment": {"method": "stub", "seed": 29},
            "dataset": {"img_dataset": img_dir or d, "prompts": os.path.join(tmp, "prompts.json"), "image_size": 64},
            "inference": {"batch_size": 2, "output_type": "latent"}}
    if params is not None:
        conf["experiment_params"] = params
    m = M(_wrap(conf))
    m.generate(m.test_dataset.batches(2), 3, 2)
    return m.model.calls


def test_harness_inpaint_box_makes_the_mask_and_defaults_the_strength(tmp_path):
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        os.environ.pop(k, None)
    calls = _harness(str(tmp_path), {"inpaint_box": [8, 16, 40, 64]})
    assert [c["image"].shape[0] for c in calls] == [2, 1]
    for c in calls:
        n = c["image"].shape[0]
        assert c["strength"] == 1.0 and c["image"].shape == (n, 3, 64, 64) and c["mask_image"].shape == (n, 1, 64, 64)
        want = torch.zeros(n, 1, 64, 64)
        want[:, :, 8:40, 16:64] = 1.0
        assert torch.equal(c["mask_image"], want)
    calls = _harness(str(tmp_path), {"inpaint_box": [8, 16, 40, 64], "strength": 0.5})
    assert all(c["strength"] == 0.5 and "mask_image" in c for c in calls)
    # the strength key alone is image-to-image, no key at all is text-to-image: unchanged
    calls = _harness(str(tmp_path), {"strength": 0.5})
    assert all("mask_image" not in c and c["strength"] == 0.5 for c in calls)
    calls = _harness(str(tmp_path), None)
    assert all("mask_image" not in c and "image" not in c and "strength" not in c for c in calls)


def test_harness_inpaint_box_errors(tmp_path):
    with pytest.raises(ValueError, match="inpaint_box"):
        _harness(str(tmp_path), {"inpaint_box": [8, 16, 40, 72]})            # past dataset.image_size
    with pytest.raises(FileNotFoundError, match="no_such_dir"):
        _harness(str(tmp_path), {"inpaint_box": [8, 16, 40, 64]}, img_dir=os.path.join(str(tmp_path), "no_such_dir"))


def test_yaml_inpaint_box_is_parsed(tmp_path):
    from sonicdiffusionbayeslab_amd.config import load_config
    from sonicdiffusionbayeslab_amd.experiments.base_experiment import BaseMethod as B
    p = tmp_path / "c.yaml"
    p.write_text("experiment_params:\n  inpaint_box: [64, 128, 256, 384]\n  strength: 0.75\ndataset:\n  image_size: 512\n")
    conf = load_config(str(p))
    assert B.parse_inpaint_box(conf.experiment_params.inpaint_box, int(conf.dataset.image_size)) == (64, 128, 256, 384)
    assert float(conf.experiment_params.strength) == 0.75
