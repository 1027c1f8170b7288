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


# 3x3 convs of the SD-1.5 UNet per level (Cin, Cout): down-block resnets, the mid block, up-block resnets over the skip
# concat; and the up-blocks' upsamplers (level -> level - 1), which the plan runs as a fused nearest-2x conv where the low-res
# pixels are not a multiple of 64 (else as the sub-pixel form, tests/test_resolution_gpu.py)
UNET_LEVEL_CONVS = {0: [(320, 320), (640, 320), (960, 320)],
                    1: [(320, 640), (640, 640), (1920, 640), (1280, 640), (960, 640)],
                    2: [(640, 1280), (1280, 1280), (2560, 1280), (1920, 1280)],
                    3: [(1280, 1280), (2560, 1280)]}
UNET_UPSAMPLERS = {3: 1280, 2: 1280, 1: 640}


def _conv_class(lib, B, H, W, Cin, Cout, up):
    """(form, kernel, split-K > 1, power-of-two output width) of a stride-1 3x3 conv, as the library selects it."""
    Ho, Wo = H << up, W << up
    kern = lib.sd_op_conv3x3_kernel(B * Ho * Wo, Cout, Cin, H, W, 1, up, 0)
    splitk = lib.sd_op_conv3x3_splitk(B * Ho * Wo, Cout, Cin, H, W, 1, up)
    assert kern in (0, 1) and splitk >= 1
    return ("upsample" if up else "conv", kern, splitk > 1, Wo & (Wo - 1) == 0)


def test_edge_conv_table_covers_every_kernel_class():
    """Every legal latent size (the size rule's image sides 256..1024 in steps of 64: latent sides 32..128, 169 sizes) at UNet batch 2 (one latent + CFG) and 32 (16 + CFG):
    each 3x3 conv of each UNet level falls in a class (form, kernel, split-K or not, power-of-two width or not).  The GPU
    parity table (tests/test_resolution_edges_gpu.py::EDGE_CONV_SHAPES) must hold a shape of every class that occurs, and
    its recorded kernels must be the ones the selection rule picks: a rule change that opens an untested class fails here."""
    from tests.test_resolution_edges_gpu import EDGE_CONV_SHAPES
    lib = _lib.load()
    model = _model()

    def legal(side):
        try:
            model.check_size(side, 512)
            return True
        except ValueError:
            return False
    sides = [s // 8 for s in range(8, 2049, 8) if legal(s)]
    assert sides == list(range(32, 129, 8))
    seen = {}
    for lh in sides:
        for lw in sides:
            for ub in (2, 32):
                for lvl, convs in UNET_LEVEL_CONVS.items():
                    for cin, cout in convs:
                        seen.setdefault(_conv_class(lib, ub, lh >> lvl, lw >> lvl, cin, cout, 0), (ub, lh, lw, lvl, cin, cout))
                for lvl, c in UNET_UPSAMPLERS.items():
                    h, w = lh >> lvl, lw >> lvl
                    if (h * w) % 64:
                        seen.setdefault(_conv_class(lib, ub, h, w, c, c, 1), (ub, lh, lw, lvl, c, c))
    tested = set()
    for B, H, W, Cin, Cout, up, kernel in EDGE_CONV_SHAPES:
        cls = _conv_class(lib, B, H, W, Cin, Cout, up)
        assert cls[1] == kernel, (B, H, W, Cin, Cout, up)
        tested.add(cls)
    missing = {c: s for c, s in seen.items() if c not in tested}
    assert not missing, f"conv classes without a GPU parity shape (class: first (batch, latent h, w, level, Cin, Cout)): {missing}"
    assert len(seen) >= 12
