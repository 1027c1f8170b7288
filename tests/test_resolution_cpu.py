"""height / width of the pipelines without a GPU: the size rule is checked before any device work, and the C ABI
exports the latent-size entry points (include/sd_hip.h; tests/test_host_cpu.py checks every declared symbol)."""
import pytest
import torch

from sonicdiffusionbayeslab_amd import _lib

NEW_SYMBOLS = ["sd_unet_workspace_bytes_hw", "sd_unet_set_context_hw", "sd_unet_forward_hw", "sd_vae_decode_hw",
               "sd_op_conv3x3_kernel", "sd_op_softmax_rows"]


def _model(sample_size=64):
    from sonicdiffusionbayeslab_amd.models import StableDiffusionModel
    from sonicdiffusionbayeslab_amd.weights import UNetConfig
    return StableDiffusionModel(unet_config=UNetConfig(sample_size=sample_size), state_dict={})


def _embeds():
    return torch.zeros(1, 77, 768), torch.zeros(1, 77, 768)


@pytest.mark.parametrize("height,width", [(500, 512), (512, 520), (192, 512), (512, 1088), (1024, 2048), (0, 512),
                                          (512.0, 768), ("512", 768)])
def test_bad_sizes_raise_before_any_gpu_use(monkeypatch, height, width):
    model = _model()

    def no_gpu(*a, **k):
        raise AssertionError("the size must be checked before the UNet is built")
    monkeypatch.setattr(model, "_ensure_unet", no_gpu)
    pe, ne = _embeds()
    with pytest.raises(ValueError, match="multiple of 64 in \\[256, 1024\\]"):
        model(prompt_embeds=pe, negative_prompt_embeds=ne, height=height, width=width, num_inference_steps=1,
              output_type="latent")


@pytest.mark.parametrize("height,width,expect", [(None, None, (512, 512)), (512, 768, (512, 768)), (768, 512, (768, 512)),
                                                 (256, 1024, (256, 1024)), (None, 640, (512, 640))])
def test_supported_sizes(height, width, expect):
    assert _model().check_size(height, width) == expect


def test_default_size_of_a_small_unet_stays_accepted():
    """sample_size * 8 is the default and accepted even outside the rule (the reduced-size configs)."""
    model = _model(16)
    assert model.check_size(None, None) == (128, 128)
    assert model.check_size(128, 128) == (128, 128)
    with pytest.raises(ValueError):
        model.check_size(128, 192)


def test_variant_pipelines_check_the_size(monkeypatch):
    from sonicdiffusionbayeslab_amd import models as M
    from sonicdiffusionbayeslab_amd.weights import UNetConfig
    pe, ne = _embeds()
    for cls, kw in [(M.StableDiffusionModelSkipTimesteps, dict(num_inference_steps=2, skip_timesteps=[])),
                    (M.StableDiffusionModelInterlivingSchedulers, dict(num_inference_steps=2, interliving_steps=[])),
                    (M.StableDiffusionModelTwoSchedulers, dict(num_inference_steps_first=2))]:
        model = cls(unet_config=UNetConfig(sample_size=64), state_dict={})
        model.scheduler_first = model.scheduler_second = model.scheduler_main = model.scheduler_inter = model.scheduler
        monkeypatch.setattr(model, "_ensure_unet", lambda: (_ for _ in ()).throw(AssertionError("GPU touched")))
        with pytest.raises(ValueError, match="multiple of 64"):
            model(prompt_embeds=pe, negative_prompt_embeds=ne, height=704, width=1100, output_type="latent", **kw)


def test_latents_must_match_the_size():
    model = _model()
    with pytest.raises(ValueError, match="do not match"):
        model.prepare_latents(1, 4, 512, 768, "cpu", None, torch.zeros(1, 4, 64, 64))


def test_new_symbols_are_exported():
    lib = _lib.load()
    for n in NEW_SYMBOLS:
        assert hasattr(lib, n), n
        assert n in _lib._SIGS, n


def test_conv3x3_kernel_selection_without_a_device():
    """sd_op_conv3x3_kernel does no device work: 0 = implicit GEMM, 1 = halo, 2 = halo 4-tap."""
    k = _lib.load().sd_op_conv3x3_kernel
    assert k(32 * 64 * 64, 320, 320, 64, 64, 1, 0, 0) == 1
    assert k(32 * 32 * 32, 640, 640, 32, 32, 1, 0, 0) == 1
    assert k(32 * 32 * 32, 320, 320, 64, 64, 2, 0, 0) == 0
    assert k(4 * 32 * 32 * 32, 640, 640, 32, 32, 1, 2, 0) == 2
    assert k(1, 1, 1, 1, 1, 3, 0, 0) < 0                    # stride 3: refused
