"""The options of the UNet and of the pipelines, and the pairs of them that are not built together -- one table for every
Python layer (``models.py``: ``enable_*`` / ``apply_tome`` and the checks of a call; ``unet.py``: the wrapper's setters and its
static ``check_*`` helpers).  GPU-free.

The first twelve names and ``HANDLE_PAIRS`` restate the table of ``csrc/model.h`` (``option_name`` / ``option_conflict``),
which the library's setters, forward and workspace sizing check; ``tests/test_options_cpu.py`` compares the two name by name
and pair by pair.  ``PIPELINE_PAIRS`` are the rows that exist above the library only.  The one parametric rule -- SAG with a
HyperTile ``max_depth`` that reaches the mid block -- is not a pair and stays where it is checked."""
from __future__ import annotations

from typing import Dict, Iterable, Optional

# the library's options, in the order of its enum: three properties of a handle, three of a forward, six settings
FP8, INPAINT9, IP_MODEL = "fp8", "9-channel UNet", "UNet with IP-Adapter weights"
DEEPCACHE, IP_PROMPT, CONTROL = "DeepCache", "IP-Adapter image prompt", "ControlNet residuals"
TOME, HYPERTILE, FREEU, TGATE, PAG, SAG = "Token Merging", "HyperTile", "FreeU", "T-GATE", "PAG", "SAG"
HANDLE_OPTIONS = (FP8, INPAINT9, IP_MODEL, DEEPCACHE, IP_PROMPT, CONTROL, TOME, HYPERTILE, FREEU, TGATE, PAG, SAG)
# ... and what only a pipeline knows
VARIANT = "the variant pipelines (two schedulers, interleaving, skipped steps)"
RESCALE = "guidance_rescale > 0"
OPTIONS = HANDLE_OPTIONS + (VARIANT, RESCALE)

HANDLE_PAIRS = {
    (FP8, CONTROL): "the calibrated activation scales do not describe the skip tensors with residuals added",
    (FP8, TOME): "the merge and unmerge kernels take bf16 tokens",
    (FP8, HYPERTILE): "the tile gather and scatter take bf16 tokens",
    (FP8, FREEU): "the calibrated activation scales do not describe the scaled tensors",
    (FP8, TGATE): "the calibrated activation scales do not describe the gated tensors",
    (FP8, PAG): "the identity kernel takes bf16 tokens",
    (FP8, SAG): "the attention-mass kernel takes bf16 q | k",
    (INPAINT9, TGATE): "an inpainting UNet is not gated",
    (INPAINT9, PAG): "an inpainting UNet has no perturbed branch",
    (INPAINT9, SAG): "the degraded latents have no mask channels",
    (IP_MODEL, TGATE): "the image branch of the cross-attention is not cached",
    (IP_MODEL, PAG): "the image prompt has no third branch",
    (IP_MODEL, SAG): "the image prompt has no branch on the degraded latents",
    (TOME, HYPERTILE): "merged tokens have no tile grid",
    (TOME, PAG): "merged tokens have no identity attention",
    (TOME, SAG): "merged tokens have no attention mass",
    (TGATE, DEEPCACHE): "the cached features are stored at the CFG batch",
    (TGATE, IP_PROMPT): "the image branch of the cross-attention is not cached",
    (TGATE, CONTROL): "the residuals are computed for the CFG batch",
    (TGATE, PAG): "behind the gate the UNet runs at the latent batch alone",
    (TGATE, SAG): "behind the gate the step has no pair to degrade from",
    (PAG, DEEPCACHE): "the cached features are stored at the CFG batch",
    (PAG, IP_PROMPT): "the image prompt has no third branch",
    (PAG, CONTROL): "the residuals are computed for the CFG batch",
    (PAG, SAG): "one extra guidance branch per step is built",
    (SAG, DEEPCACHE): "a skip step does not run the mid block",
    (SAG, IP_PROMPT): "the image prompt has no branch on the degraded latents",
    (SAG, CONTROL): "the residuals are computed for the first forward alone",
    (CONTROL, DEEPCACHE): "a skip step does not run the blocks the residuals are added in",
}
PIPELINE_PAIRS = {
    (VARIANT, TGATE): "their step lists are not one schedule to place a gate in; StableDiffusionModel runs it",
    (VARIANT, PAG): "their history hand-off combines a CFG pair, not three branches; StableDiffusionModel runs it",
    (VARIANT, SAG): "their history hand-off combines a CFG pair, not the SAG prediction; StableDiffusionModel runs it",
    (SAG, RESCALE): "upstream's SAG pipeline has no rescale",
}
_REFUSED: Dict[frozenset, str] = {frozenset(k): v for k, v in {**HANDLE_PAIRS, **PIPELINE_PAIRS}.items()}

# the way out a refusal names, per layer: how the option that is on goes off
MODEL_OFF = {TOME: "remove_tome()", HYPERTILE: "disable_hypertile()", FREEU: "disable_freeu()", TGATE: "disable_tgate()",
             PAG: "disable_pag()", SAG: "disable_sag()", DEEPCACHE: "disable the DeepCache helper",
             CONTROL: "unload_controlnet()", IP_PROMPT: "unload_ip_adapter()"}
HANDLE_OFF = {TOME: "set_tome(0.0)", HYPERTILE: "set_hypertile(0)", FREEU: "disable_freeu()", TGATE: "set_tgate(TGATE_OFF)",
              PAG: "set_pag(0)", SAG: "set_sag(False)", DEEPCACHE: "set_deepcache(-1)", CONTROL: "clear_control_residuals()",
              IP_PROMPT: "clear_ip_adapter()"}


def conflict(a: str, b: str) -> Optional[str]:
    """Why options ``a`` and ``b`` are refused together; None when the pair is built.  Symmetric."""
    return _REFUSED.get(frozenset((a, b)))


def check(asked: str, on: Iterable[str], way_out: Dict[str, str] = MODEL_OFF) -> None:
    """``asked`` is about to go on beside the options ``on``: ``NotImplementedError`` naming both, the reason and the way out
    for the first of them (in the order of ``OPTIONS``) it is refused with."""
    on = set(on)
    for other in OPTIONS:
        why = conflict(asked, other) if other in on else None
        if why is not None:
            hint = f" ({way_out[other]} first)" if other in way_out else ""
            raise NotImplementedError(f"{asked} with {other} is not built: {why}{hint}")


def handle_options(config=None, weight_dtype: str = "bf16") -> list:
    """The options a UNet handle has by construction: its weight dtype, a 9-channel input, IP-Adapter weights."""
    from ._lib import DTYPE_FP8_E4M3, DTYPES
    on = [FP8] if DTYPES.get(weight_dtype) == DTYPE_FP8_E4M3 else []
    if config is not None and config.in_channels == 9:
        on.append(INPAINT9)
    if config is not None and getattr(config, "ip_adapter_embed_dim", None) is not None:
        on.append(IP_MODEL)
    return on
