"""The tiny autoencoder (AutoencoderTiny / TAESD) without a GPU: the parameter table (Python and library), the config refusals,
the oracle (tests/taesd_oracle.py) against answers that can be worked out by hand, the synthetic stand-in's conditions, the
host logic of ``load_tiny_vae`` / ``unload_tiny_vae`` / ``use_for``, the YAML keys, and the image-to-image draw order."""
import ctypes as C
import json
import math
import os

import pytest
import torch
import torch.nn.functional as F

from sonicdiffusionbayeslab_amd import _lib
from sonicdiffusionbayeslab_amd.vae import (TinyVaeConfig, check_tiny_vae_config, load_tiny_vae_state_dict,
                                            make_synthetic_tiny_vae_state_dict, tiny_vae_decoder_param_shapes,
                                            tiny_vae_encoder_param_shapes, tiny_vae_param_shapes)
from tests import taesd_oracle as O

NEW_SYMBOLS = ["sd_taesd_decoder_create", "sd_taesd_encoder_create", "sd_taesd_decode_hw", "sd_taesd_encode_hw", "sd_op_conv64",
               "sd_op_conv64_pack", "sd_op_taesd_entry", "sd_op_taesd_exit"]


def test_new_symbols_are_exported_and_the_abi_version_stays():
    lib = _lib.load()
    for n in NEW_SYMBOLS:
        assert hasattr(lib, n), n
        assert n in _lib._SIGS and n in _lib.declared_symbols(), n
    assert lib.sd_abi_version() == 3


# ---------------------------------------------------------------- parameter table
def _block(p):
    out = []
    for k in (0, 2, 4):
        out += [(f"{p}conv.{k}.weight", (64, 64, 3, 3)), (f"{p}conv.{k}.bias", (64,))]
    return out


def _w(p):
    return [(p + "weight", (64, 64, 3, 3))]


E, D = "encoder.layers.", "decoder.layers."
# diffusers 0.32 AutoencoderTiny state-dict names and shapes, written out layer by layer (upstream-recall)
TAESD_ENCODER = ([(E + "0.weight", (64, 3, 3, 3)), (E + "0.bias", (64,))] + _block(E + "1.") + _w(E + "2.")
                 + _block(E + "3.") + _block(E + "4.") + _block(E + "5.") + _w(E + "6.")
                 + _block(E + "7.") + _block(E + "8.") + _block(E + "9.") + _w(E + "10.")
                 + _block(E + "11.") + _block(E + "12.") + _block(E + "13.")
                 + [(E + "14.weight", (4, 64, 3, 3)), (E + "14.bias", (4,))])
TAESD_DECODER = ([(D + "0.weight", (64, 4, 3, 3)), (D + "0.bias", (64,))] + _block(D + "2.") + _block(D + "3.") + _block(D + "4.")
                 + _w(D + "6.") + _block(D + "7.") + _block(D + "8.") + _block(D + "9.") + _w(D + "11.")
                 + _block(D + "12.") + _block(D + "13.") + _block(D + "14.") + _w(D + "16.") + _block(D + "17.")
                 + [(D + "18.weight", (3, 64, 3, 3)), (D + "18.bias", (3,))])


def test_param_shapes_are_the_diffusers_table():
    assert tiny_vae_encoder_param_shapes() == TAESD_ENCODER
    assert tiny_vae_decoder_param_shapes() == TAESD_DECODER
    shapes = tiny_vae_param_shapes(TinyVaeConfig())
    assert shapes == TAESD_ENCODER + TAESD_DECODER
    assert len(shapes) == 134
    assert sum(math.prod(s) for _, s in shapes) == 2445063


def _enumerate(create):
    lib = _lib.load()
    h = C.c_void_p()
    _lib.check(getattr(lib, create)(C.byref(h)))
    try:
        got = []
        for i in range(lib.sd_unet_num_params(h)):
            name, shape, nd = C.create_string_buffer(256), (C.c_longlong * 4)(), C.c_int()
            _lib.check(lib.sd_unet_param_info(h, i, name, 256, shape, C.byref(nd)))
            got.append((name.value.decode(), tuple(shape[k] for k in range(nd.value))))
        # the workspace is three activation buffers of the largest level; sizes outside the rule are refused
        assert lib.sd_unet_workspace_bytes_hw(h, 2, -1, 8, 16) == 3 * 2 * 64 * 128 * 64 * 2
        assert lib.sd_unet_workspace_bytes_hw(h, 2, -1, 8, 12) < 0 and b"multiples of 8" in lib.sd_last_error()
        assert lib.sd_unet_workspace_bytes_hw(h, 1, -1, 136, 8) < 0
    finally:
        lib.sd_unet_destroy(h)
    return got


def test_library_enumerates_the_same_table():
    """Host only: no device is touched before finalize."""
    assert _enumerate("sd_taesd_decoder_create") == TAESD_DECODER
    assert _enumerate("sd_taesd_encoder_create") == TAESD_ENCODER


def test_oracle_loads_the_state_dict_strictly():
    sd = make_synthetic_tiny_vae_state_dict()
    assert list(sd) == [n for n, _ in tiny_vae_param_shapes()]
    m = O.build(sd)                                          # load_state_dict(strict=True): the key table
    assert sorted(m.state_dict()) == sorted(sd)
    bad = dict(sd)
    bad["decoder.layers.5.weight"] = bad.pop("decoder.layers.6.weight")
    with pytest.raises(RuntimeError):
        O.build(bad)
    for v in sd.values():                                    # on the bf16 grid
        assert torch.equal(v, v.to(torch.bfloat16).float())


# ---------------------------------------------------------------- config refusals
@pytest.mark.parametrize("key,value", [("latent_channels", 16), ("act_fn", "silu"), ("upsample_fn", "bilinear"),
                                       ("num_encoder_blocks", [1, 3, 3]), ("num_decoder_blocks", [3, 3, 3, 3]),
                                       ("encoder_block_out_channels", [64, 64, 64, 128]),
                                       ("decoder_block_out_channels", [128, 64, 64, 64]), ("scaling_factor", 0.18215),
                                       ("in_channels", 1), ("out_channels", 4)])
def test_other_structures_are_refused_by_name(key, value):
    base = {"_class_name": "AutoencoderTiny", "act_fn": "relu", "latent_channels": 4, "upsample_fn": "nearest",
            "num_encoder_blocks": [1, 3, 3, 3], "num_decoder_blocks": [3, 3, 3, 1], "scaling_factor": 1.0,
            "encoder_block_out_channels": [64, 64, 64, 64], "decoder_block_out_channels": [64, 64, 64, 64]}
    assert check_tiny_vae_config(base) == TinyVaeConfig()
    with pytest.raises(NotImplementedError, match=key):
        check_tiny_vae_config({**base, key: value})
    with pytest.raises(NotImplementedError, match=key):
        tiny_vae_param_shapes(TinyVaeConfig(**{key: tuple(value) if isinstance(value, list) else value}))


def test_local_directory_is_read_and_checked_strictly(tmp_path):
    from safetensors.torch import save_file
    sd = make_synthetic_tiny_vae_state_dict(seed=9)
    d = tmp_path / "taesd"
    d.mkdir()
    (d / "config.json").write_text(json.dumps({"_class_name": "AutoencoderTiny", "latent_channels": 4, "act_fn": "relu"}))
    save_file({k: v.to(torch.float16) for k, v in sd.items()}, str(d / "diffusion_pytorch_model.safetensors"))
    got = load_tiny_vae_state_dict(str(d))
    assert sorted(got) == sorted(sd) and all(v.dtype == torch.float32 for v in got.values())
    (d / "config.json").write_text(json.dumps({"latent_channels": 16}))
    with pytest.raises(NotImplementedError, match="latent_channels"):
        load_tiny_vae_state_dict(str(d))
    (d / "config.json").write_text("{}")
    short = {k: v for k, v in sd.items() if k != "encoder.layers.2.weight"}
    save_file(short, str(d / "diffusion_pytorch_model.safetensors"))
    with pytest.raises(KeyError, match="encoder.layers.2.weight"):
        load_tiny_vae_state_dict(str(d))
    save_file({**sd, "decoder.layers.6.bias": torch.zeros(64)}, str(d / "diffusion_pytorch_model.safetensors"))
    with pytest.raises(KeyError, match="decoder.layers.6.bias"):
        load_tiny_vae_state_dict(str(d))
    save_file({**sd, "decoder.layers.18.weight": torch.zeros(4, 64, 3, 3)}, str(d / "diffusion_pytorch_model.safetensors"))
    with pytest.raises(ValueError, match="decoder.layers.18.weight"):
        load_tiny_vae_state_dict(str(d))
    with pytest.raises(FileNotFoundError):
        load_tiny_vae_state_dict(str(tmp_path / "nowhere"))


# ---------------------------------------------------------------- oracle, by hand
def test_block_with_zero_convs_is_relu():
    blk = O.AutoencoderTinyBlock(64, 64)
    for p in blk.parameters():
        torch.nn.init.zeros_(p)
    x = torch.randn(2, 64, 5, 7, generator=torch.Generator().manual_seed(1))
    with torch.no_grad():
        assert torch.equal(blk(x), F.relu(x))


def _centre_identity(c):
    w = torch.zeros(c, c, 3, 3)
    w[torch.arange(c), torch.arange(c), 1, 1] = 1.0
    return w


def test_upsample_then_centre_tap_identity_is_the_nearest_upsampled_input():
    dec = O.DecoderTiny()
    up, conv = dec.layers[5], dec.layers[6]
    assert isinstance(up, torch.nn.Upsample) and conv.bias is None
    with torch.no_grad():
        conv.weight.copy_(_centre_identity(64))
        x = torch.randn(1, 64, 3, 5, generator=torch.Generator().manual_seed(2))
        y = conv(up(x))
    assert y.shape == (1, 64, 6, 10)
    for yy in range(6):
        for xx in range(10):
            assert torch.equal(y[0, :, yy, xx], x[0, :, yy // 2, xx // 2])


def test_stride_two_conv_picks_even_pixels_with_pad_one_on_all_sides():
    enc = O.EncoderTiny()
    conv = enc.layers[2]
    assert conv.stride == (2, 2) and conv.padding == (1, 1) and conv.bias is None
    x = torch.randn(1, 64, 8, 12, generator=torch.Generator().manual_seed(3))
    with torch.no_grad():
        conv.weight.copy_(_centre_identity(64))
        assert torch.equal(conv(x), x[:, :, 0::2, 0::2])             # pixels (0,0), (0,2), ...
        # the top-left tap reads (2y - 1, 2x - 1): zero padding on the TOP and LEFT (not the AutoencoderKL's right / bottom)
        w = torch.zeros(64, 64, 3, 3)
        w[torch.arange(64), torch.arange(64), 0, 0] = 1.0
        conv.weight.copy_(w)
        y = conv(x)
    assert torch.equal(y[:, :, 0, :], torch.zeros(1, 64, 6)) and torch.equal(y[:, :, :, 0], torch.zeros(1, 64, 4))
    assert torch.equal(y[:, :, 1:, 1:], x[:, :, 1:-1:2, 1:-1:2])


def test_decoder_input_squash_and_output_range():
    z = torch.tensor([0.0, 3.0, -3.0, 30.0, -30.0])
    got = torch.tanh(z / 3) * 3
    want = torch.tensor([0.0, 3 * math.tanh(1.0), -3 * math.tanh(1.0), 3.0, -3.0])
    assert torch.allclose(got, want, atol=1e-6) and got[0] == 0 and got.abs().max() <= 3
    # a decoder whose convs are all zero but the exit bias: tanh squash in, y * 2 - 1 out
    dec = O.DecoderTiny()
    for p in dec.parameters():
        torch.nn.init.zeros_(p)
    with torch.no_grad():
        dec.layers[18].bias.copy_(torch.tensor([0.0, 0.5, 1.0]))
        y = dec(torch.randn(1, 4, 2, 2))
    assert y.shape == (1, 3, 16, 16)
    for c, v in enumerate((-1.0, 0.0, 1.0)):
        assert torch.equal(y[0, c], torch.full((16, 16), v))


def test_encoder_takes_the_unit_range_image():
    """``encode01`` is the pipeline's 2 x - 1 followed by the model's (x + 1) / 2: the entry conv sees the [0, 1] image."""
    m = O.build(make_synthetic_tiny_vae_state_dict())
    img = torch.rand(1, 3, 64, 64, generator=torch.Generator().manual_seed(5))
    with torch.no_grad():
        direct = m.encoder.layers(img)
    got = m.encode01(img)
    assert got.shape == (1, 4, 8, 8)
    assert (got - direct).abs().max() < 1e-4 * direct.abs().max()


# ---------------------------------------------------------------- the stand-in
TEST_LATENTS = (((2, 4, 8, 8), 5), ((2, 4, 16, 24), 6))        # (shape, seed) of tests/test_taesd_gpu.py's parity cases


def test_standin_picture_is_mid_grey_with_spread_and_few_clamped_pixels():
    """The 64 -> 3 exit's factor (vae.TINY_EXIT_IMAGE_FACTOR): fewer than 2 % of the pixels outside [0, 1] and a std of at
    least 0.1, for the default seed and the latents the GPU tests decode."""
    m = O.build(make_synthetic_tiny_vae_state_dict())
    for shape, seed in TEST_LATENTS:
        z = torch.randn(shape, generator=torch.Generator().manual_seed(seed))
        pic = m.decode(z) / 2 + 0.5
        outside = float(((pic < 0) | (pic > 1)).float().mean())
        print(f"stand-in {shape}: mean {float(pic.mean()):.3f} std {float(pic.std()):.3f} outside {outside:.4f}")
        assert outside < 0.02 and float(pic.std()) >= 0.1 and 0.4 < float(pic.mean()) < 0.6


def test_standin_activations_stay_in_range():
    """Every stored activation of either half stays within a factor of ~10 of unit scale (bf16 has the range; what
    matters is that nothing dies or blows up through 35 convs)."""
    m = O.build(make_synthetic_tiny_vae_state_dict())
    z = torch.randn((2, 4, 16, 24), generator=torch.Generator().manual_seed(6))
    img = torch.rand((2, 3, 128, 192), generator=torch.Generator().manual_seed(7))
    with torch.no_grad():
        for half, x in ((m.decoder, torch.tanh(z / 3) * 3), (m.encoder, img)):
            for layer in half.layers[:-1]:
                x = layer(x)
                if isinstance(layer, (O.AutoencoderTinyBlock, O._Conv)):
                    assert 0.2 < float(x.std()) < 12.0, (type(layer).__name__, float(x.std()))
    assert 0.2 < float(m.encode01(img).std()) < 8.0


# ---------------------------------------------------------------- load_tiny_vae / unload_tiny_vae, host logic
def _model(sample_size=16):
    from sonicdiffusionbayeslab_amd.models import StableDiffusionModel
    from sonicdiffusionbayeslab_amd.registry import schedulers_registry
    from sonicdiffusionbayeslab_amd.weights import UNetConfig
    m = StableDiffusionModel(unet_config=UNetConfig(sample_size=sample_size), state_dict={})
    m.scheduler = schedulers_registry["ddim_scheduler"].from_config(m.scheduler.config)
    return m


def test_load_and_unload_host_logic(tmp_path):
    m = _model()
    src0 = m.weights_source
    assert m.tiny_vae_use is None
    with pytest.raises(ValueError, match="use_for"):
        m.load_tiny_vae("madebyollin/taesd", use_for="final")
    with pytest.raises(FileNotFoundError):
        m.load_tiny_vae(str(tmp_path / "no" / "such" / "dir"))
    assert m.tiny_vae_use is None and m.weights_source == src0
    m.load_tiny_vae("madebyollin/taesd")
    assert m.tiny_vae_use == "all"
    assert "SYNTHETIC stand-in for the hub AutoencoderTiny madebyollin/taesd" in m.weights_source
    with pytest.raises(NotImplementedError, match="already loaded"):
        m.load_tiny_vae("madebyollin/taesd", use_for="previews")
    m.unload_tiny_vae()
    assert m.tiny_vae_use is None and m.weights_source == src0 and m.tiny_vae_decoder is None and m.tiny_vae_encoder is None
    m.load_tiny_vae("madebyollin/taesd", use_for="previews")
    assert m.tiny_vae_use == "previews" and "previews" in m.weights_source
    m.unload_tiny_vae()
    m.unload_tiny_vae()                                      # idempotent
    # a local directory is read for real
    from safetensors.torch import save_file
    d = tmp_path / "taesd"
    d.mkdir()
    (d / "config.json").write_text(json.dumps({"latent_channels": 4}))
    sd = make_synthetic_tiny_vae_state_dict(seed=3)
    save_file(sd, str(d / "diffusion_pytorch_model.safetensors"))
    m.load_tiny_vae(str(d))
    assert f"AutoencoderTiny(local:{d}" in m.weights_source
    assert torch.equal(m._tiny_state_dict()["decoder.layers.0.weight"], sd["decoder.layers.0.weight"])


class _Decoder:
    """Stands in for either decoder: a constant picture per latent, so that the caller can tell which one ran."""
    def __init__(self, value, log):
        self.value, self.log = value, log

    def decode(self, latents, *a, **kw):
        self.log.append((self.value, kw.get("unit_range", None), tuple(latents.shape)))
        return torch.full((latents.shape[0], 3, 8 * latents.shape[2], 8 * latents.shape[3]), self.value)


def test_finish_routes_by_use_for(monkeypatch):
    m = _model()
    log = []
    kl, tiny = _Decoder(0.5, log), _Decoder(0.25, log)
    monkeypatch.setattr(m, "_ensure_vae", lambda: kl)
    monkeypatch.setattr(m, "_ensure_tiny_vae", lambda: tiny)
    lat, x0 = torch.zeros(2, 4, 16, 16), [torch.zeros(1, 4, 16, 16)] * 3
    out, _, prev = m._finish(lat, x0, "pt", True, 0.0)          # nothing loaded: today's path
    assert torch.equal(out.images, torch.full((2, 3, 128, 128), 0.75)) and len(prev) == 3
    assert all(v == 0.5 and ur is None for v, ur, _ in log) and len(log) == 4
    log.clear()
    m.load_tiny_vae("madebyollin/taesd", use_for="previews")
    out, _, prev = m._finish(lat, x0, "pt", True, 0.0)
    assert torch.equal(out.images, torch.full((2, 3, 128, 128), 0.75))               # the final image: AutoencoderKL, / 2 + 0.5
    assert all(torch.equal(p, torch.full((1, 3, 128, 128), 0.25)) for p in prev)     # previews: tiny, unit range as it is
    assert [(v, ur) for v, ur, _ in log] == [(0.5, None)] + [(0.25, True)] * 3
    log.clear()
    m.unload_tiny_vae()
    m.load_tiny_vae("madebyollin/taesd", use_for="all")
    out, _, prev = m._finish(lat, x0, "np", True, 0.0)
    assert out.images.shape == (2, 128, 128, 3) and float(out.images.max()) == 0.25 and len(prev) == 3
    assert [(v, ur) for v, ur, _ in log] == [(0.25, True)] * 4
    out, _, _ = m._finish(lat, x0, "latent", True, 0.0)
    assert out.images is lat
    log.clear()
    m.unload_tiny_vae()
    m._finish(lat, x0, "pt", True, 0.0)
    assert all(v == 0.5 for v, _, _ in log)


class _Encoder:
    def __init__(self, log):
        self.log = log

    def encode(self, img, *a, **kw):
        self.log.append("tiny")
        return torch.zeros(img.shape[0], 4, img.shape[2] // 8, img.shape[3] // 8)


def test_img2img_draw_order_with_the_tiny_encoder(monkeypatch):
    """No posterior Gaussian is drawn: the forward noise is the generator's FIRST draw, whatever ``sample_mode`` says."""
    m = _model()
    log, seen = [], {}
    monkeypatch.setattr(m, "_ensure_tiny_vae_encoder", lambda: _Encoder(log))
    monkeypatch.setattr(m, "_ensure_vae_encoder", lambda: (_ for _ in ()).throw(AssertionError("the AutoencoderKL encoder must not run")))
    monkeypatch.setattr(m.scheduler, "add_noise", lambda init, noise, t: seen.update(init=init, noise=noise) or init + noise)
    m.load_tiny_vae("madebyollin/taesd", use_for="all")
    img = torch.rand(2, 3, 128, 192)
    for mode in ("sample", "argmax"):
        g, g2 = torch.Generator().manual_seed(17), torch.Generator().manual_seed(17)
        start, init = m._img2img_start(img, mode, g, "cpu", 500)
        first = torch.randn(2, 4, 16, 24, generator=g2)
        assert torch.equal(seen["noise"], first) and torch.equal(g.get_state(), g2.get_state())
        assert torch.equal(init, torch.zeros(2, 4, 16, 24)) and torch.equal(start, first)
    assert log == ["tiny", "tiny"]


def test_previews_keep_encoding_on_the_autoencoder_kl(monkeypatch):
    m = _model()
    m.load_tiny_vae("madebyollin/taesd", use_for="previews")
    monkeypatch.setattr(m, "_ensure_tiny_vae_encoder", lambda: (_ for _ in ()).throw(AssertionError("previews only")))

    class KL:
        def encode(self, img):
            return torch.zeros(img.shape[0], 8, img.shape[2] // 8, img.shape[3] // 8)

        def sample(self, moments, noise, mode="sample", scale=None):
            return moments[:, :4] if noise is None else noise

    monkeypatch.setattr(m, "_ensure_vae_encoder", lambda: KL())
    g, g2 = torch.Generator().manual_seed(3), torch.Generator().manual_seed(3)
    lat = m._image_latents(torch.rand(1, 3, 128, 128), (1, 4, 16, 16), "sample", g)
    assert torch.equal(lat, torch.randn(1, 4, 16, 16, generator=g2))        # the posterior draw comes first, as before


# ---------------------------------------------------------------- YAML
def _harness(tmp, model_keys):
    from sonicdiffusionbayeslab_amd.config import _wrap
    from sonicdiffusionbayeslab_amd.experiments.base_experiment import BaseMethod

    class M(BaseMethod):
        def setup_scheduler(self, **kw):
            pass

        def run_experiment(self):
            pass

    conf = {"experiment_name": "stub", "experiment": {"method": "stub", "seed": 29},
            "model": {"model_name": "stable_diffusion_model", "pretrained_model": "runwayml/stable-diffusion-v1-5", **model_keys},
            "dataset": {"img_dataset": os.path.join(tmp, "img"), "prompts": os.path.join(tmp, "prompts.json"), "image_size": 64},
            "inference": {"batch_size": 3, "output_type": "latent"}, "experiment_params": {}}
    return M(_wrap(conf))


def test_yaml_keys(tmp_path):
    from tests.test_img2img_cpu import _write_dataset
    tmp = str(tmp_path)
    _write_dataset(tmp)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        os.environ.pop(k, None)
    m = _harness(tmp, {"tiny_vae": "madebyollin/taesd"})
    assert m.model.tiny_vae_use == "all" and "AutoencoderTiny madebyollin/taesd" in m.model.weights_source
    m = _harness(tmp, {"tiny_vae": "madebyollin/taesd", "tiny_vae_use": "previews"})
    assert m.model.tiny_vae_use == "previews"
    m = _harness(tmp, {})
    assert m.model.tiny_vae_use is None and "AutoencoderTiny" not in m.model.weights_source
    with pytest.raises(ValueError, match="use_for"):
        _harness(tmp, {"tiny_vae": "madebyollin/taesd", "tiny_vae_use": "everything"})


def test_the_shipped_config_is_the_lcm_config_plus_the_key():
    from sonicdiffusionbayeslab_amd.config import load_config
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    tiny = load_config(os.path.join(root, "configs", "tiny_vae_config.yaml"))
    lcm = load_config(os.path.join(root, "configs", "lcm_distilled_config.yaml"))
    assert tiny.model.tiny_vae == "madebyollin/taesd" and tiny.model.tiny_vae_use == "all"
    assert tiny.model.pretrained_model == lcm.model.pretrained_model and tiny.model.time_cond_proj_dim == lcm.model.time_cond_proj_dim
    assert tiny.scheduler.scheduler_name == lcm.scheduler.scheduler_name
    assert list(tiny.experiment_params.num_inference_steps) == list(lcm.experiment_params.num_inference_steps)
    assert tiny.inference.batch_size == lcm.inference.batch_size
