"""Image-to-image without a GPU: the encoder's exports and parameter table, the synthetic stand-in's decoder stream, the
fp32 oracle (tests/vae_encoder_oracle.py) against closed forms, the strength -> (t_start, steps) table, every argument
check before any GPU work, the Pillow transform and the harness key ``experiment_params.strength``."""
import hashlib
import json
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp
import torch.nn.functional as F

from sonicdiffusionbayeslab_amd import _lib

NEW_SYMBOLS = ["sd_vae_encoder_create", "sd_vae_encode_hw", "sd_vae_posterior_sample", "sd_op_conv3x3_down_asym"]


def test_encoder_symbols_are_exported_and_the_abi_version_stays():
    lib = _lib.load()
    for n in NEW_SYMBOLS:
        assert hasattr(lib, n), n
        assert n in _lib._SIGS and n in _lib.declared_symbols(), n
    assert lib.sd_abi_version() == 3


def _resnet(p, cin, cout):
    out = [(p + "norm1.weight", (cin,)), (p + "norm1.bias", (cin,)), (p + "conv1.weight", (cout, cin, 3, 3)),
           (p + "conv1.bias", (cout,)), (p + "norm2.weight", (cout,)), (p + "norm2.bias", (cout,)),
           (p + "conv2.weight", (cout, cout, 3, 3)), (p + "conv2.bias", (cout,))]
    if cin != cout:
        out += [(p + "conv_shortcut.weight", (cout, cin, 1, 1)), (p + "conv_shortcut.bias", (cout,))]
    return out


# diffusers 0.32.1 AutoencoderKL state-dict names and shapes of the SD-1.5 VAE's encoder half, in module order
SD15_ENCODER = (
    [("encoder.conv_in.weight", (128, 3, 3, 3)), ("encoder.conv_in.bias", (128,))]
    + _resnet("encoder.down_blocks.0.resnets.0.", 128, 128) + _resnet("encoder.down_blocks.0.resnets.1.", 128, 128)
    + [("encoder.down_blocks.0.downsamplers.0.conv.weight", (128, 128, 3, 3)), ("encoder.down_blocks.0.downsamplers.0.conv.bias", (128,))]
    + _resnet("encoder.down_blocks.1.resnets.0.", 128, 256) + _resnet("encoder.down_blocks.1.resnets.1.", 256, 256)
    + [("encoder.down_blocks.1.downsamplers.0.conv.weight", (256, 256, 3, 3)), ("encoder.down_blocks.1.downsamplers.0.conv.bias", (256,))]
    + _resnet("encoder.down_blocks.2.resnets.0.", 256, 512) + _resnet("encoder.down_blocks.2.resnets.1.", 512, 512)
    + [("encoder.down_blocks.2.downsamplers.0.conv.weight", (512, 512, 3, 3)), ("encoder.down_blocks.2.downsamplers.0.conv.bias", (512,))]
    + _resnet("encoder.down_blocks.3.resnets.0.", 512, 512) + _resnet("encoder.down_blocks.3.resnets.1.", 512, 512)
    + _resnet("encoder.mid_block.resnets.0.", 512, 512)
    + [("encoder.mid_block.attentions.0.group_norm.weight", (512,)), ("encoder.mid_block.attentions.0.group_norm.bias", (512,)),
       ("encoder.mid_block.attentions.0.to_q.weight", (512, 512)), ("encoder.mid_block.attentions.0.to_q.bias", (512,)),
       ("encoder.mid_block.attentions.0.to_k.weight", (512, 512)), ("encoder.mid_block.attentions.0.to_k.bias", (512,)),
       ("encoder.mid_block.attentions.0.to_v.weight", (512, 512)), ("encoder.mid_block.attentions.0.to_v.bias", (512,)),
       ("encoder.mid_block.attentions.0.to_out.0.weight", (512, 512)), ("encoder.mid_block.attentions.0.to_out.0.bias", (512,))]
    + _resnet("encoder.mid_block.resnets.1.", 512, 512)
    + [("encoder.conv_norm_out.weight", (512,)), ("encoder.conv_norm_out.bias", (512,)),
       ("encoder.conv_out.weight", (8, 512, 3, 3)), ("encoder.conv_out.bias", (8,)),
       ("quant_conv.weight", (8, 8, 1, 1)), ("quant_conv.bias", (8,))])


def test_encoder_param_shapes_are_the_diffusers_table():
    import ctypes as C
    from sonicdiffusionbayeslab_amd.vae import VaeConfig, _c_config, vae_encoder_param_shapes
    cfg = VaeConfig()
    assert vae_encoder_param_shapes(cfg) == SD15_ENCODER
    assert sum(torch.Size(s).numel() for _, s in SD15_ENCODER) == 34163664          # 34.2 M parameters
    # the library enumerates the same table (host only: no device is touched before finalize)
    lib = _lib.load()
    h = C.c_void_p()
    _lib.check(lib.sd_vae_encoder_create(C.byref(_c_config(cfg)), C.byref(h)))
    try:
        got = []
        for i in range(lib.sd_unet_num_params(h)):
            name, shape, nd = C.create_string_buffer(256), (C.c_longlong * 4)(), C.c_int()
            _lib.check(lib.sd_unet_param_info(h, i, name, 256, shape, C.byref(nd)))
            got.append((name.value.decode(), tuple(shape[k] for k in range(nd.value))))
    finally:
        lib.sd_unet_destroy(h)
    assert got == SD15_ENCODER


# sha256 over (name, fp32 bytes) of the decoder tensors of make_synthetic_vae_state_dict(VaeConfig()) in vae_param_shapes
# order, taken on the commit before the encoder existed
DECODER_DIGEST = "2f96f52c4083910e922f2a060f714ddba7304afa8486b792ca9b747b15bb0217"


def test_synthetic_decoder_tensors_did_not_move():
    from sonicdiffusionbayeslab_amd.vae import (SYNTHETIC_LOGVAR_BIAS, VaeConfig, make_synthetic_vae_state_dict,
                                                vae_encoder_param_shapes, vae_param_shapes)
    cfg = VaeConfig()
    sd = make_synthetic_vae_state_dict(cfg)
    h = hashlib.sha256()
    for n, _ in vae_param_shapes(cfg):
        h.update(n.encode())
        h.update(sd[n].numpy().tobytes())
    assert h.hexdigest() == DECODER_DIGEST
    for n, s in vae_encoder_param_shapes(cfg):
        assert tuple(sd[n].shape) == s, n
    assert (sd["quant_conv.bias"][4:] == SYNTHETIC_LOGVAR_BIAS).all() and SYNTHETIC_LOGVAR_BIAS < 0


def test_oracle_downsampler_is_pad_right_bottom_then_unpadded_stride_2():
    from tests.vae_encoder_oracle import downsample
    g = torch.Generator().manual_seed(3)
    for h, w in ((8, 8), (6, 10)):
        x, wt, b = torch.randn(2, 5, h, w, generator=g), torch.randn(7, 5, 3, 3, generator=g), torch.randn(7, generator=g)
        want = F.conv2d(F.pad(x, (0, 1, 0, 1)), wt, b, stride=2)
        assert want.shape == (2, 7, h // 2, w // 2)
        assert torch.equal(downsample(x, wt, b), want)
        # written out: output (oy, ox) reads input rows 2oy .. 2oy+2, columns 2ox .. 2ox+2, zero past the edge
        xp = torch.zeros(2, 5, h + 1, w + 1); xp[:, :, :h, :w] = x
        oy, ox = h // 2 - 1, w // 2 - 1
        val = (xp[:, :, 2 * oy:2 * oy + 3, 2 * ox:2 * ox + 3][:, None] * wt[None]).sum((2, 3, 4)) + b
        assert torch.allclose(want[:, :, oy, ox], val, atol=1e-5)
        # and it is NOT the symmetric pad-1 stride-2 conv of the UNet
        assert not torch.allclose(want, F.conv2d(x, wt, b, stride=2, padding=1))


def test_oracle_posterior_sample_is_the_closed_form_with_both_clamps():
    from tests.vae_encoder_oracle import posterior_sample
    mean = torch.tensor([0.5, -1.0, 2.0, 0.25]).view(1, 4, 1, 1)
    logvar = torch.tensor([-40.0, 25.0, 0.0, -2.0]).view(1, 4, 1, 1)
    eps = torch.tensor([1.0, -2.0, 0.5, 3.0]).view(1, 4, 1, 1)
    got = posterior_sample(torch.cat([mean, logvar], 1), eps, "sample", 0.18215).double().flatten()
    import math
    want = [0.18215 * (0.5 + math.exp(-15.0) * 1.0), 0.18215 * (-1.0 + math.exp(10.0) * -2.0),
            0.18215 * (2.0 + 1.0 * 0.5), 0.18215 * (0.25 + math.exp(-1.0) * 3.0)]
    for g, w in zip(got.tolist(), want):
        assert abs(g - w) <= 2e-6 * abs(w), (g, w)
    assert torch.equal(posterior_sample(torch.cat([mean, logvar], 1), None, "argmax", 2.0), 2.0 * mean)


# (N, strength) -> (t_start, steps run), written out by hand from init = min(int(N s), N), t_start = max(N - init, 0);
# None: fewer than one step -> ValueError
STRENGTH_TABLE = {
    (1, 0.0): None, (1, 0.02): None, (1, 0.5): None, (1, 0.8): None, (1, 1.0): (0, 1),
    (4, 0.0): None, (4, 0.02): None, (4, 0.5): (2, 2), (4, 0.8): (1, 3), (4, 1.0): (0, 4),
    (20, 0.0): None, (20, 0.02): None, (20, 0.5): (10, 10), (20, 0.8): (4, 16), (20, 1.0): (0, 20),
    (50, 0.0): None, (50, 0.02): (49, 1), (50, 0.5): (25, 25), (50, 0.8): (10, 40), (50, 1.0): (0, 50),
}


def _model(sample_size=64):
    from sonicdiffusionbayeslab_amd.models import StableDiffusionModel
    from sonicdiffusionbayeslab_amd.registry import schedulers_registry
    from sonicdiffusionbayeslab_amd.weights import UNetConfig
    m = StableDiffusionModel(unet_config=UNetConfig(sample_size=sample_size), state_dict={})
    m.scheduler = schedulers_registry["ddim_scheduler"].from_config(m.scheduler.config)
    return m


def test_strength_table():
    from sonicdiffusionbayeslab_amd.models import StableDiffusionModel as M
    for (n, s), want in STRENGTH_TABLE.items():
        if want is None:
            with pytest.raises(ValueError, match="at least one"):
                M.img2img_steps(n, s)
        else:
            assert M.img2img_steps(n, s) == want, (n, s)
    for bad in (-0.1, 1.01, float("nan"), "0.5", None):
        with pytest.raises(ValueError, match="strength"):
            M.img2img_steps(20, bad)


def _no_gpu(model, monkeypatch):
    def boom(*a, **k):
        raise AssertionError("the arguments must be checked before the UNet is built")
    monkeypatch.setattr(model, "_ensure_unet", boom)


def test_image_argument_errors_come_before_any_gpu_work(monkeypatch):
    from sonicdiffusionbayeslab_amd.registry import schedulers_registry
    model = _model()
    _no_gpu(model, monkeypatch)
    pe = torch.zeros(1, 77, 768)
    img = torch.rand(1, 3, 512, 768)
    call = lambda **kw: model(**{**dict(prompt_embeds=pe, negative_prompt_embeds=pe, image=img, num_inference_steps=10,
                                        output_type="latent"), **kw})
    with pytest.raises(ValueError, match="exclusive"):
        call(latents=torch.zeros(1, 4, 64, 96))
    with pytest.raises(ValueError, match="strength"):
        call(strength=1.5)
    with pytest.raises(ValueError, match="strength"):
        call(strength=-0.01)
    with pytest.raises(ValueError, match="at least one"):
        call(strength=0.05)
    with pytest.raises(ValueError, match="disagrees"):
        call(height=512, width=512)
    with pytest.raises(ValueError, match="disagrees"):
        call(height=768)
    with pytest.raises(ValueError, match="multiple of 64 in \\[256, 1024\\]"):
        call(image=torch.rand(1, 3, 500, 512))
    with pytest.raises(ValueError, match="multiple of 64 in \\[256, 1024\\]"):
        call(image=torch.rand(1, 3, 128, 512))
    with pytest.raises(ValueError, match="prompt batch"):
        call(image=torch.rand(2, 3, 512, 512))
    with pytest.raises(ValueError, match="float tensor"):
        call(image=torch.zeros(1, 3, 512, 512, dtype=torch.uint8))
    with pytest.raises(ValueError, match="float tensor"):
        call(image=torch.rand(3, 512, 512))
    with pytest.raises(ValueError, match="sample_mode"):
        call(sample_mode="mean")
    from PIL import Image
    with pytest.raises(ValueError, match="one size"):
        model(["a", "b"], image=[Image.new("RGB", (512, 512)), Image.new("RGB", (768, 512))], num_inference_steps=10)
    # agreeing height / width and a well-formed call get as far as the UNet
    with pytest.raises(AssertionError, match="before the UNet is built"):
        call(height=512, width=768)
    with pytest.raises(AssertionError, match="before the UNet is built"):
        model(["a"], image=[Image.new("RGB", (768, 512))], num_inference_steps=10, strength=0.5)
    # PNDM (the checkpoint's scheduler) is refused by name, on the new argument only
    from sonicdiffusionbayeslab_amd.schedulers import PNDMConfigStub
    model.scheduler = schedulers_registry["pndm_scheduler"].from_config(PNDMConfigStub().config)
    with pytest.raises(NotImplementedError, match="PNDMScheduler"):
        call()


def test_variant_pipelines_refuse_an_image(monkeypatch):
    from sonicdiffusionbayeslab_amd import models as M
    from sonicdiffusionbayeslab_amd.weights import UNetConfig
    pe = torch.zeros(1, 77, 768)
    img = torch.rand(1, 3, 512, 512)
    for cls, kw in [(M.StableDiffusionModelSkipTimesteps, dict(num_inference_steps=2, skip_timesteps=[])),
                    (M.StableDiffusionModelInterlivingSchedulers, dict(num_inference_steps=2, interliving_steps=[])),
                    (M.StableDiffusionModelTwoSchedulers, dict(num_inference_steps_first=2))]:
        model = cls(unet_config=UNetConfig(sample_size=64), state_dict={})
        model.scheduler_first = model.scheduler_second = model.scheduler_main = model.scheduler_inter = model.scheduler
        _no_gpu(model, monkeypatch)
        with pytest.raises(NotImplementedError, match="image"):
            model(prompt_embeds=pe, negative_prompt_embeds=pe, image=img, output_type="latent", **kw)


def test_pil_images_become_unit_range_tensors():
    from PIL import Image
    from sonicdiffusionbayeslab_amd.models import StableDiffusionModel as M
    a = Image.new("RGB", (4, 2), (255, 0, 51))
    t = M._image_tensor([a, a])
    assert t.shape == (2, 3, 2, 4) and t.dtype == torch.float32
    assert torch.equal(t[0, :, 0, 0], torch.tensor([1.0, 0.0, 51 / 255.0]))


def _gradient(w, h):
    """RGB image whose red channel is the column index and whose green channel is the row index (mod 256)."""
    import numpy as np
    from PIL import Image
    a = np.zeros((h, w, 3), dtype=np.uint8)
    a[..., 0] = (np.arange(w) % 256)[None, :]
    a[..., 1] = (np.arange(h) % 256)[:, None]
    a[..., 2] = 200
    return Image.fromarray(a)


@pytest.mark.parametrize("w,h,size,resized", [(640, 480, 256, (341, 256)), (300, 500, 128, (128, 213)), (512, 512, 512, (512, 512))])
def test_pillow_transform_sizes_and_centre(w, h, size, resized):
    """Resize(size) (shorter side -> size, longer -> int(size * long / short), bilinear), CenterCrop(size), ToTensor()."""
    import numpy as np
    from PIL import Image
    from sonicdiffusionbayeslab_amd.dataset import image_transform
    img = _gradient(w, h)
    t = image_transform(img, size)
    assert t.shape == (3, size, size) and t.dtype == torch.float32 and 0.0 <= float(t.min()) and float(t.max()) <= 1.0
    rw, rh = resized
    assert (rw, rh) == ((size, int(size * h / w)) if w <= h else (int(size * w / h), size))
    left, top = int(round((rw - size) / 2.0)), int(round((rh - size) / 2.0))
    want = np.asarray(img.resize((rw, rh), Image.BILINEAR), dtype=np.float32)[top:top + size, left:left + size] / 255.0
    assert torch.equal(t, torch.from_numpy(want).permute(2, 0, 1))
    assert torch.all(t[2] == 200 / 255.0)
    # centred: as many resized columns / rows are cut on one side as on the other, to within the one of an odd remainder
    assert abs((rw - size - left) - left) <= 1 and abs((rh - size - top) - top) <= 1


# ---------------------------------------------------------------------------------------------------
# harness: experiment_params.strength -> every prompt's own file is loaded, sliced per rank with the prompts
# ---------------------------------------------------------------------------------------------------
class _StubOut:
    def __init__(self, images):
        self.images = images


class _StubPipeline:
    """A per-image function of (prompt, start image, the two Gaussians an image-to-image call draws)."""
    weights_source = "stub"
    num_timesteps = 3

    def __init__(self):
        from sonicdiffusionbayeslab_amd.schedulers import SchedulerConfig
        from sonicdiffusionbayeslab_amd.weights import UNetConfig
        self.unet_config = UNetConfig(sample_size=8)
        self.scheduler = type("S", (), {})()
        self.scheduler.config = SchedulerConfig()
        self.seen = []

    def to(self, device):
        return self

    def __call__(self, prompts, num_inference_steps=3, guidance_scale=7.5, generator=None, output_type="latent",
                 image=None, strength=None, **kw):
        from sonicdiffusionbayeslab_amd import dist as sdist
        n = len(prompts)
        assert image is not None and image.shape == (n, 3, 64, 64) and strength == 0.5
        post = sdist.randn((n, 4, 8, 8), generator)
        noise = sdist.randn((n, 4, 8, 8), generator)
        enc = F.avg_pool2d(image, 8)[:, :1].expand(n, 4, 8, 8)
        key = torch.tensor([float(sum(map(ord, p)) % 97) for p in prompts]).view(n, 1, 1, 1)
        self.seen.append(n)
        return _StubOut(enc + 0.1 * post + strength * noise + key), 0.25, []


def _write_dataset(tmp, n=5):
    from PIL import Image
    os.makedirs(os.path.join(tmp, "img"), exist_ok=True)
    prompts = {}
    for i in range(n):
        name = f"im{i}.png"
        Image.new("RGB", (96 + 8 * i, 80), (40 * i, 255 - 30 * i, 7 * i)).save(os.path.join(tmp, "img", name))
        prompts[name] = f"prompt number {i}"
    with open(os.path.join(tmp, "prompts.json"), "w") as f:
        json.dump(prompts, f)
    return os.path.join(tmp, "img"), os.path.join(tmp, "prompts.json")


def _harness_run(tmp, strength=0.5, img_dir=None, pipeline=None):
    from sonicdiffusionbayeslab_amd.config import _wrap
    from sonicdiffusionbayeslab_amd.experiments.base_experiment import BaseMethod

    class M(BaseMethod):
        def setup_model(self):
            self.model = (pipeline or _StubPipeline)()

        def setup_scheduler(self, **kw):
            pass

        def run_experiment(self):
            pass

    d, p = os.path.join(tmp, "img"), os.path.join(tmp, "prompts.json")
    conf = {"experiment_name": "stub", "experiment": {"method": "stub", "seed": 29},
            "dataset": {"img_dataset": img_dir or d, "prompts": p, "image_size": 64},
            "inference": {"batch_size": 3, "output_type": "latent"}}
    if strength is not None:
        conf["experiment_params"] = {"strength": strength}
    m = M(_wrap(conf))
    m.test_dataset.image_files = sorted(m.test_dataset.image_files)
    images, _ = m.generate(m.test_dataset.batches(3), 3, 3)
    return torch.stack(images), list(m.model.seen)


def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close(); return p


def _harness_worker(rank, world, port, tmp, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank), SD_DIST_BACKEND="gloo")
    out, seen = _harness_run(tmp)
    q.put((rank, out.numpy(), seen))
    dist.barrier()
    dist.destroy_process_group()


def test_harness_strength_key_loads_and_shards_the_images(tmp_path):
    tmp = str(tmp_path)
    _write_dataset(tmp)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        os.environ.pop(k, None)
    want, seen = _harness_run(tmp)
    assert want.shape == (5, 4, 8, 8) and seen == [3, 2]
    # the images matter: image i is a flat colour whose red channel is 40 i / 255
    from sonicdiffusionbayeslab_amd.dataset import load_image
    assert abs(float(load_image(os.path.join(tmp, "img", "im2.png"), 64)[0].mean()) - 80 / 255.0) < 1e-6
    # two ranks over gloo: every rank ends with the single-process result, every image computed once
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


def test_harness_strength_with_a_missing_directory_names_it(tmp_path):
    tmp = str(tmp_path)
    _write_dataset(tmp)
    missing = os.path.join(tmp, "no_such_dir")
    with pytest.raises(FileNotFoundError, match="no_such_dir"):
        _harness_run(tmp, img_dir=missing)


def test_harness_without_the_key_opens_no_image(tmp_path, monkeypatch):
    from sonicdiffusionbayeslab_amd.experiments import base_experiment as BE
    tmp = str(tmp_path)
    _write_dataset(tmp)
    monkeypatch.setattr(BE, "load_image", lambda *a, **k: (_ for _ in ()).throw(AssertionError("an image was opened")))

    class P(_StubPipeline):
        def __call__(self, prompts, image=None, strength=None, **kw):
            assert image is None and strength is None
            return _StubOut(torch.zeros(len(prompts), 4, 8, 8)), 0.1, []
    out, _ = _harness_run(tmp, strength=None, img_dir=os.path.join(tmp, "no_such_dir"), pipeline=P)
    assert out.shape == (5, 4, 8, 8)
