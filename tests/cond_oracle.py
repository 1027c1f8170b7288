"""The CPU oracle for LCM-distilled UNets (``time_cond_proj_dim``): diffusers' ``TimestepEmbedding.forward(t_emb, condition)``
adds ``cond_proj(condition)`` to the timestep sinusoid before ``linear_1``.  ``oracle.unet.unet_forward`` looks up the
module-level ``timestep_embedding`` on every call, so replacing that function conditions every oracle forward -- also the
loops of ``oracle/pipeline.py`` (call those with ``guidance_scale <= 1``: they derive CFG from it, and a conditioned UNet
runs without CFG).  The condition is the product's host embedding of ``guidance_scale - 1`` (tested against float64 in
tests/test_guidance_embed_cpu.py); the projection runs in fp32 on the bf16-grid weight."""
import contextlib

import torch.nn.functional as F

import oracle.unet as ounet
from sonicdiffusionbayeslab_amd.models import get_guidance_scale_embedding

COND = "time_embedding.cond_proj.weight"


def cond_row(sd, guidance_scale):
    """[1, c0] = cond_proj . get_guidance_scale_embedding(guidance_scale - 1)."""
    w = sd[COND].float()
    return F.linear(get_guidance_scale_embedding(float(guidance_scale) - 1.0, w.shape[1]), w)


@contextlib.contextmanager
def conditioned_oracle(sd, guidance_scale):
    """Within the block every oracle UNet forward embeds ``guidance_scale`` through ``sd``'s cond_proj."""
    row = cond_row(sd, guidance_scale)
    plain = ounet.timestep_embedding

    def timestep_embedding(t, dim=320):
        return plain(t, dim) + row

    ounet.timestep_embedding = timestep_embedding
    try:
        yield row
    finally:
        ounet.timestep_embedding = plain
