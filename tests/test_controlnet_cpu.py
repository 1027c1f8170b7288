"""ControlNet without a GPU: the oracle (tests/controlnet_oracle.py) against oracle.unet, the synthetic weights' gain, the
``keep`` schedule, the config reader, the exported symbols and every refusal of the pipeline call."""
import ctypes as C
import json

import pytest
import torch

from sonicdiffusionbayeslab_amd import _lib
from sonicdiffusionbayeslab_amd.weights import (CONTROLNET_EMBED_CHANNELS, ControlNetConfig, UNetConfig, control_keep,
                                                controlnet_config_for, controlnet_param_shapes, controlnet_residual_shapes,
                                                make_synthetic_controlnet_state_dict, make_synthetic_state_dict,
                                                read_controlnet_config)
from tests.controlnet_oracle import controlnet_forward, unet_forward_with_residuals
from tests.util import oracle_cfg, rel_l2

UNET_TOL = 2e-2                     # tests/test_unet_gpu.py

NEW_SYMBOLS = ["sd_controlnet_create", "sd_controlnet_residual_bytes_hw", "sd_controlnet_set_cond_hw", "sd_controlnet_forward_hw",
               "sd_unet_set_control_residuals_hw", "sd_op_conv_in_add", "sd_op_residual_add"]

# config.json of lllyasviel/sd-controlnet-canny (the values this build reads; upstream-recall)
SD15_CONTROLNET_CONFIG = {
    "_class_name": "ControlNetModel", "act_fn": "silu", "attention_head_dim": 8, "block_out_channels": [320, 640, 1280, 1280],
    "class_embed_type": None, "conditioning_embedding_out_channels": [16, 32, 96, 256], "controlnet_conditioning_channel_order": "rgb",
    "cross_attention_dim": 768, "down_block_types": ["CrossAttnDownBlock2D", "CrossAttnDownBlock2D", "CrossAttnDownBlock2D", "DownBlock2D"],
    "downsample_padding": 1, "flip_sin_to_cos": True, "freq_shift": 0, "in_channels": 4, "layers_per_block": 2,
    "mid_block_scale_factor": 1, "norm_eps": 1e-05, "norm_num_groups": 32, "num_class_embeds": None, "only_cross_attention": False,
    "projection_class_embeddings_input_dim": None, "resnet_time_scale_shift": "default", "upcast_attention": False,
    "use_linear_projection": False, "global_pool_conditions": False, "conditioning_channels": 3,
}


@pytest.fixture(scope="module")
def weights():
    cfg = UNetConfig(sample_size=32)
    cn = controlnet_config_for(cfg)
    return cfg, make_synthetic_state_dict(cfg, seed=1234), cn, make_synthetic_controlnet_state_dict(cn, seed=1234)


def _inputs(h, w, seed=29):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(1, 4, h, w, generator=g), torch.randn(1, 77, 768, generator=g), torch.rand(1, 3, 8 * h, 8 * w, generator=g))


@pytest.mark.parametrize("h,w", [(32, 32), (32, 40)])
def test_restated_unet_with_zero_residuals_is_the_oracle_bit_for_bit(weights, h, w):
    from oracle.unet import unet_forward
    cfg, sd, cn, _ = weights
    lat, pe, _ = _inputs(h, w)
    oc = oracle_cfg(cfg)
    zeros = [torch.zeros(1, c, hh, ww) for c, hh, ww in controlnet_residual_shapes(cn, h, w)]
    with torch.no_grad():
        ref = unet_forward(sd, oc, lat, 981.0, pe)
        got = unet_forward_with_residuals(sd, oc, lat, 981.0, pe, zeros[:-1], zeros[-1])
        none = unet_forward_with_residuals(sd, oc, lat, 981.0, pe)
    assert torch.equal(got, ref) and torch.equal(none, ref)


def test_controlnet_oracle_shapes_and_order_at_32x40(weights):
    cfg, sd, cn, cw = weights
    lat, pe, cond = _inputs(32, 40)
    with torch.no_grad():
        down, mid = controlnet_forward(cw, oracle_cfg(cfg), lat, 499.0, pe, cond)
    want = [(320, 32, 40)] * 3 + [(320, 16, 20)] + [(640, 16, 20)] * 2 + [(640, 8, 10)] + [(1280, 8, 10)] * 2 + [(1280, 4, 5)] + \
           [(1280, 4, 5)] * 2
    assert len(down) == 12 and [tuple(d.shape[1:]) for d in down] == want and tuple(mid.shape) == (1, 1280, 4, 5)
    assert controlnet_residual_shapes(cn, 32, 40) == want + [(1280, 4, 5)]
    assert all(torch.isfinite(d).all() and d.abs().max() > 0 for d in down + [mid])      # synthetic zero convs are not zero


@pytest.mark.parametrize("t", [981.0, 21.0])
def test_synthetic_controlnet_moves_eps(weights, t):
    """Fixes ``gain`` of make_synthetic_controlnet_state_dict: at its default the residuals at scale 1.0 move the oracle's
    eps by more than 10 x UNET_TOL at both ends of the schedule (measured: 0.47 at t = 981, 0.45 at t = 21; a gain of 0.25
    gives 0.26 / 0.24, too close to the 0.2 the GPU tests ask for)."""
    cfg, sd, cn, cw = weights
    lat, pe, cond = _inputs(32, 32)
    oc = oracle_cfg(cfg)
    with torch.no_grad():
        down, mid = controlnet_forward(cw, oc, lat, t, pe, cond)
        on = unet_forward_with_residuals(sd, oc, lat, t, pe, down, mid)
        off = unet_forward_with_residuals(sd, oc, lat, t, pe)
    apart = rel_l2(on, off)
    print(f"oracle eps with residuals at scale 1.0 vs without, t={t}: rel-L2 {apart:.3f}")
    assert apart > 10 * UNET_TOL


def test_keep_schedule_against_a_hand_written_table():
    assert control_keep(4, 0.0, 1.0) == [1.0, 1.0, 1.0, 1.0]
    assert control_keep(4, 0.0, 0.5) == [1.0, 1.0, 0.0, 0.0]
    assert control_keep(4, 0.25, 0.75) == [0.0, 1.0, 1.0, 0.0]


def test_symbols_are_exported_and_the_abi_version_stays():
    lib = _lib.load()
    for n in NEW_SYMBOLS:
        assert hasattr(lib, n), n
        assert n in _lib._SIGS and n in _lib.declared_symbols(), n
    assert lib.sd_abi_version() == 3


def test_library_enumerates_the_controlnet_parameters_and_refuses_fp8():
    from sonicdiffusionbayeslab_amd.unet import _c_config
    lib = _lib.load()
    cn = controlnet_config_for(UNetConfig(sample_size=32))
    embed = (C.c_int * 4)(*cn.conditioning_embedding_out_channels)
    h = C.c_void_p()
    _lib.check(lib.sd_controlnet_create(C.byref(_c_config(cn.unet)), embed, C.byref(h)))
    try:
        name, shape, nd = C.create_string_buffer(256), (C.c_longlong * 4)(), C.c_int()
        got = []
        for i in range(lib.sd_unet_num_params(h)):
            _lib.check(lib.sd_unet_param_info(h, i, name, 256, shape, C.byref(nd)))
            got.append((name.value.decode(), tuple(shape[:nd.value])))
        assert got == controlnet_param_shapes(cn) and len(got) == 340
        from sonicdiffusionbayeslab_amd.controlnet import residual_layout
        for ub, hh, ww in ((1, 32, 32), (4, 32, 40), (16, 64, 64)):
            assert lib.sd_controlnet_residual_bytes_hw(h, ub, hh, ww) == residual_layout(cn, ub, hh, ww)[1]
    finally:
        lib.sd_unet_destroy(h)
    h2 = C.c_void_p()
    assert lib.sd_controlnet_create(C.byref(_c_config(cn.unet, "fp8")), embed, C.byref(h2)) != 0
    assert b'weight_dtype="fp8"' in lib.sd_last_error()
    from sonicdiffusionbayeslab_amd.controlnet import HipControlNetModel
    with pytest.raises(NotImplementedError, match="fp8"):
        HipControlNetModel(cn, {}, weight_dtype="fp8")


def test_read_controlnet_config():
    ucfg = UNetConfig()
    cn = read_controlnet_config(SD15_CONTROLNET_CONFIG, ucfg)
    assert cn.conditioning_embedding_out_channels == CONTROLNET_EMBED_CHANNELS and cn == controlnet_config_for(ucfg)
    assert read_controlnet_config({}, ucfg) == cn                      # every key at its SD-1.5 default
    with pytest.raises(NotImplementedError, match="global_pool_conditions"):
        read_controlnet_config({**SD15_CONTROLNET_CONFIG, "global_pool_conditions": True}, ucfg)
    with pytest.raises(NotImplementedError, match="controlnet_conditioning_channel_order"):
        read_controlnet_config({**SD15_CONTROLNET_CONFIG, "controlnet_conditioning_channel_order": "bgr"}, ucfg)
    with pytest.raises(ValueError, match="block_out_channels"):
        read_controlnet_config({**SD15_CONTROLNET_CONFIG, "block_out_channels": [320, 640, 1280, 2560]}, ucfg)
    with pytest.raises(ValueError, match="cross_attention_dim"):
        read_controlnet_config({**SD15_CONTROLNET_CONFIG, "cross_attention_dim": 1024}, ucfg)
    with pytest.raises(NotImplementedError, match="conditioning_embedding_out_channels"):
        read_controlnet_config({**SD15_CONTROLNET_CONFIG, "conditioning_embedding_out_channels": [16, 32, 96]}, ucfg)
    lcm = UNetConfig(time_cond_proj_dim=256)                           # an LCM-distilled UNet pairs with a plain ControlNet
    assert read_controlnet_config(SD15_CONTROLNET_CONFIG, lcm).unet.time_cond_proj_dim is None


def test_load_controlnet_reads_a_local_directory(tmp_path):
    from safetensors.torch import save_file
    from sonicdiffusionbayeslab_amd.registry import models_registry
    from sonicdiffusionbayeslab_amd.weights import load_controlnet
    small = UNetConfig(sample_size=16, block_out_channels=(64, 128), attn_levels=(False, False), layers_per_block=1,
                       cross_attention_dim=64, num_heads=2)
    cn = controlnet_config_for(small)
    sd = make_synthetic_controlnet_state_dict(cn, seed=3)
    cj = {**SD15_CONTROLNET_CONFIG, "block_out_channels": [64, 128], "down_block_types": ["DownBlock2D", "DownBlock2D"],
          "layers_per_block": 1, "cross_attention_dim": 64, "attention_head_dim": 2}
    (tmp_path / "config.json").write_text(json.dumps(cj))
    save_file({k: v.to(torch.bfloat16).contiguous() for k, v in sd.items()}, str(tmp_path / "diffusion_pytorch_model.safetensors"))
    got_cfg, got_sd = load_controlnet(str(tmp_path), small)
    assert got_cfg.unet.block_out_channels == (64, 128) and set(got_sd) == set(sd)
    assert all(torch.equal(got_sd[k], sd[k]) for k in sd)
    m = models_registry["stable_diffusion_model"](unet_config=small)
    m.load_controlnet(str(tmp_path))
    assert "ControlNet(local:" in m.weights_source
    with pytest.raises(NotImplementedError, match="already loaded"):
        m.load_controlnet(str(tmp_path))
    m.unload_controlnet()
    assert "ControlNet" not in m.weights_source
    with pytest.raises(ValueError, match="does not match the UNet"):
        models_registry["stable_diffusion_model"](unet_config=UNetConfig()).load_controlnet(str(tmp_path))
    with pytest.raises(FileNotFoundError):
        m.load_controlnet(str(tmp_path / "missing" / "dir"))


def _model(key="stable_diffusion_model", load=True, **kw):
    from sonicdiffusionbayeslab_amd.registry import models_registry
    m = models_registry[key](**kw)
    if load:
        m.load_controlnet("lllyasviel/sd-controlnet-canny")
        assert "SYNTHETIC stand-in for the hub ControlNet" in m.weights_source
    return m


def test_every_call_level_refusal_raises_before_any_gpu_work():
    """No GPU on this side of the suite: each call below must raise its own error by name, not the missing device's."""
    from sonicdiffusionbayeslab_amd.deepcache import DeepCacheSDHelper
    img = torch.rand(1, 3, 512, 512)
    pe = torch.zeros(1, 77, 768)
    kw = dict(prompt_embeds=pe, num_inference_steps=2, output_type="latent")
    with pytest.raises(NotImplementedError, match="Multi-ControlNet"):
        _model(load=False).load_controlnet(["a/b", "c/d"])
    m = _model()
    with pytest.raises(NotImplementedError, match="Multi-ControlNet"):
        m(control_image=[img, img], **kw)                                         # a list of images
    with pytest.raises(NotImplementedError, match="Multi-ControlNet"):
        m(control_image=[[img]], **kw)
    with pytest.raises(NotImplementedError, match="controlnet_conditioning_scale"):
        m(control_image=img, controlnet_conditioning_scale=[1.0, 0.5], **kw)      # a list of scales
    with pytest.raises(NotImplementedError, match="control_guidance_end"):
        m(control_image=img, control_guidance_end=[1.0], **kw)
    with pytest.raises(NotImplementedError, match="guess_mode"):
        m(control_image=img, guess_mode=True, **kw)
    with pytest.raises(NotImplementedError, match="mask_image"):
        m(control_image=img, image=img, mask_image=torch.ones(1, 1, 512, 512), **kw)
    with pytest.raises(ValueError, match="control_guidance_start"):
        m(control_image=img, control_guidance_start=0.6, control_guidance_end=0.5, **kw)
    with pytest.raises(ValueError, match="batch 2 does not match"):
        m(control_image=torch.rand(2, 3, 512, 512), **kw)
    with pytest.raises(ValueError, match="float tensor"):
        m(control_image=(img * 255).to(torch.uint8), **kw)
    helper = DeepCacheSDHelper(pipe=m)
    helper.set_params(cache_interval=2, cache_branch_id=0)
    helper.enable()
    try:
        with pytest.raises(NotImplementedError, match="DeepCache"):
            m(control_image=img, **kw)
    finally:
        helper.disable()
    with pytest.raises(NotImplementedError, match="fp8"):
        _model(weight_dtype="fp8")(control_image=img, **kw)
    for key in ("stable_diffusion_model_two_schedulers", "stable_diffusion_model_interliving_schedulers",
                "stable_diffusion_model_skip_timesteps"):
        with pytest.raises(NotImplementedError, match="ControlNet"):
            _model(key)(control_image=img, **kw)
    with pytest.raises(ValueError, match="needs a loaded ControlNet"):
        _model(load=False)(control_image=img, **kw)
    m.unload_controlnet()
    with pytest.raises(ValueError, match="needs a loaded ControlNet"):
        m(control_image=img, **kw)


def test_control_image_is_resized_and_sharded_like_the_other_per_sample_arguments():
    from sonicdiffusionbayeslab_amd.models import StableDiffusionModel as M
    img = torch.rand(4, 3, 64, 96, generator=torch.Generator().manual_seed(1))
    assert M.resize_control_image(img, 64, 96) is img
    up = M.resize_control_image(img, 128, 192)
    assert torch.equal(up, torch.nn.functional.interpolate(img, size=(128, 192))) and torch.equal(up[:, :, ::2, ::2], img)
    pil = M.resize_control_image(img, 128, 192, pil=True)
    assert tuple(pil.shape) == (4, 3, 128, 192) and 0.0 <= float(pil.min()) and float(pil.max()) <= 1.0
    cut = M.shard_control_args({"control_image": img, "x": 1}, 1, 3, 4)
    assert torch.equal(cut["control_image"], img[1:3]) and cut["x"] == 1
    one = M.shard_control_args({"control_image": img[:1]}, 1, 3, 4)
    assert one["control_image"].shape[0] == 1                          # a batch of 1 is broadcast and stays
    assert M.shard_control_args({"control_image": list("abcd")}, 2, 4, 4)["control_image"] == ["c", "d"]


# ---------------------------------------------------------------------------------------------------------------------
# harness: model.controlnet, experiment_params.control_from_dataset / controlnet_conditioning_scale
# ---------------------------------------------------------------------------------------------------------------------
class _ControlStub:
    """A per-image function of (prompt, control image, scale, the Gaussian a text-to-image call draws)."""
    weights_source = "stub"
    num_timesteps = 3

    def __init__(self):
        from sonicdiffusionbayeslab_amd.schedulers import SchedulerConfig
        self.unet_config = UNetConfig(sample_size=8)
        self.scheduler = type("S", (), {})()
        self.scheduler.config = SchedulerConfig()
        self.seen = []

    @staticmethod
    def shard_control_args(kw, lo, hi, n):
        from sonicdiffusionbayeslab_amd.models import StableDiffusionModel
        return StableDiffusionModel.shard_control_args(kw, lo, hi, n)

    def to(self, device):
        return self

    def __call__(self, prompts, num_inference_steps=3, guidance_scale=7.5, generator=None, output_type="latent",
                 control_image=None, controlnet_conditioning_scale=None, image=None, **kw):
        from sonicdiffusionbayeslab_amd import dist as sdist
        n = len(prompts)
        assert image is None and control_image is not None and tuple(control_image.shape) == (n, 3, 64, 64)
        assert controlnet_conditioning_scale == 0.7
        noise = sdist.randn((n, 4, 8, 8), generator)
        enc = torch.nn.functional.avg_pool2d(control_image, 8)[:, :1].expand(n, 4, 8, 8)
        key = torch.tensor([float(sum(map(ord, p)) % 97) for p in prompts]).view(n, 1, 1, 1)
        self.seen.append(n)
        return type("O", (), {"images": controlnet_conditioning_scale * enc + noise + key})(), 0.25, []


def _harness(tmp, params, model=None, controlnet="lllyasviel/sd-controlnet-canny", stub=True):
    import os
    from sonicdiffusionbayeslab_amd.config import _wrap
    from sonicdiffusionbayeslab_amd.experiments.base_experiment import BaseMethod

    class M(BaseMethod):
        def setup_model(self):
            if stub:
                self.model = _ControlStub()
            else:
                BaseMethod.setup_model(self)

        def setup_scheduler(self, **kw):
            pass

        def run_experiment(self):
            pass

    conf = {"experiment_name": "stub", "experiment": {"method": "stub", "seed": 29},
            "model": {"model_name": "stable_diffusion_model", "pretrained_model": "runwayml/stable-diffusion-v1-5"},
            "dataset": {"img_dataset": os.path.join(tmp, "img"), "prompts": os.path.join(tmp, "prompts.json"), "image_size": 64},
            "inference": {"batch_size": 3, "output_type": "latent"}, "experiment_params": params}
    if controlnet is not None:
        conf["model"]["controlnet"] = controlnet
    m = M(_wrap(conf))
    m.test_dataset.image_files = sorted(m.test_dataset.image_files)
    return m


def _harness_run(tmp):
    m = _harness(tmp, {"control_from_dataset": True, "controlnet_conditioning_scale": 0.7})
    images, _ = m.generate(m.test_dataset.batches(3), 3, 3)
    return torch.stack(images), list(m.model.seen)


def _harness_worker(rank, world, port, tmp, q):
    import os
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank), SD_DIST_BACKEND="gloo")
    out, seen = _harness_run(tmp)
    q.put((rank, out.numpy(), seen))
    dist.barrier()
    dist.destroy_process_group()


def test_harness_control_from_dataset_loads_and_shards_the_control_images(tmp_path):
    """Every prompt's own file is its control image at the configured scale; two ranks over gloo end with the single-process
    result, every image computed once from ITS file (the stub's output depends on the control image)."""
    import os
    import torch.multiprocessing as mp
    from tests.test_img2img_cpu import _free_port, _write_dataset
    tmp = str(tmp_path)
    _write_dataset(tmp)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        os.environ.pop(k, None)
    want, seen = _harness_run(tmp)
    assert want.shape == (5, 4, 8, 8) and seen == [3, 2]
    assert (want[1] - want[0]).abs().max() > 0                         # different files, different outputs
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    ps = [ctx.Process(target=_harness_worker, args=(r, 2, port, tmp, q)) for r in range(2)]
    [p.start() for p in ps]
    outs = {r: (torch.from_numpy(a), s) for r, a, s in (q.get(timeout=300) for _ in range(2))}
    [p.join(60) for p in ps]
    assert all(p.exitcode == 0 for p in ps)
    for r in (0, 1):
        assert torch.equal(outs[r][0], want), r
    assert sum(outs[0][1]) + sum(outs[1][1]) == 5


def test_harness_keys_and_their_refusals(tmp_path):
    import os
    from tests.test_img2img_cpu import _write_dataset
    tmp = str(tmp_path)
    _write_dataset(tmp)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        os.environ.pop(k, None)
    m = _harness(tmp, {}, stub=False)                                   # model.controlnet: loaded before the model moves
    assert "SYNTHETIC stand-in for the hub ControlNet lllyasviel/sd-controlnet-canny" in m.model.weights_source
    assert m.control_from_dataset is False and m.controlnet_conditioning_scale == 1.0
    plain = _harness(tmp, {}, controlnet=None, stub=False)
    assert "ControlNet" not in plain.model.weights_source
    with pytest.raises(ValueError, match="model.controlnet"):
        _harness(tmp, {"control_from_dataset": True}, controlnet=None)
    with pytest.raises(NotImplementedError, match="inpaint_box"):
        _harness(tmp, {"control_from_dataset": True, "inpaint_box": [0, 0, 32, 32]})
    os.rename(os.path.join(tmp, "img"), os.path.join(tmp, "moved"))
    with pytest.raises(FileNotFoundError, match="control_from_dataset"):
        _harness(tmp, {"control_from_dataset": True})
