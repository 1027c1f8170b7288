"""The operator entry points of the text / vision towers' small kernels (sd_op_clip_embed, sd_op_activation, sd_op_pool_rows,
sd_op_vit_embed) are exported and bound, and the constant tests/test_encoder_ops_gpu.py relies on for the exact GELU --
bounds.GELU_POLY, the 1.3e-5 |x| of csrc/common.h::gelu_erf_f -- holds for the formula itself.  No GPU needed."""
import math

import numpy as np
import torch

from sonicdiffusionbayeslab_amd import _lib
from tests.bounds import GELU_POLY

NEW_OPS = ("sd_op_clip_embed", "sd_op_activation", "sd_op_pool_rows", "sd_op_vit_embed")


def bf16_finite_zero_or_normal():
    """Every bf16 bit pattern that is finite and zero or normal, as float32: 65536 - 256 inf / NaN - 254 subnormals."""
    bits = np.arange(65536, dtype=np.uint32)
    exp, man = (bits >> 7) & 0xFF, bits & 0x7F
    keep = (exp != 0xFF) & ((exp != 0) | (man == 0))
    x = (bits[keep] << 16).astype(np.uint32).view(np.float32)
    assert x.size == 65026
    return x


def test_encoder_operator_symbols_are_exported_and_the_abi_version_stays(sdlib):
    declared = _lib.declared_symbols()
    for n in NEW_OPS:
        assert hasattr(sdlib, n), f"{n} is not exported"
        assert n in _lib._SIGS, f"{n} has no signature in _lib._SIGS"
        assert n in declared, f"{n} is not declared in include/sd_hip.h"
    assert sdlib.sd_abi_version() == 3


def gelu_erf_f32(x):
    """csrc/common.h::gelu_erf_f in float32, one rounding per operation (the fused multiply-add through float64: the product of
    two float32 values is exact there), with an exact reciprocal and exp2 in place of v_rcp_f32 / v_exp_f32."""
    f = np.float32
    z = np.abs(x) * f(0.70710678118654752)
    t = (f(1.0) / (f(0.47047).astype(np.float64) * z.astype(np.float64) + 1.0).astype(np.float32)).astype(np.float32)
    poly = t * (f(0.3480242) + t * (f(-0.0958798) + t * f(0.7478556)))
    e = np.exp2(z * z * f(-1.4426950408889634)).astype(np.float32)
    half_erfc = f(0.5) * poly * e
    phi = np.where(x < 0, half_erfc, f(1.0) - half_erfc).astype(np.float32)
    return (x * phi).astype(np.float32)


def test_gelu_erf_formula_stays_within_gelu_poly_of_the_exact_gelu():
    """|gelu_erf_f(x) - x Phi(x)| <= GELU_POLY |x| over every finite zero-or-normal bf16 input; measured maximum
    1.095e-5 |x| at x = 2.328125 (GELU_POLY = 1.3e-5)."""
    x = bf16_finite_zero_or_normal()
    with np.errstate(over="ignore", under="ignore"):
        got = gelu_erf_f32(x).astype(np.float64)
    xd = torch.from_numpy(x.astype(np.float64))
    ref = (xd * 0.5 * torch.special.erfc(-xd / math.sqrt(2.0))).numpy()
    assert np.isfinite(got).all() and np.isfinite(ref).all()
    nz = x != 0
    assert (got[~nz] == 0).all()
    ratio = np.abs(got[nz] - ref[nz]) / np.abs(x[nz].astype(np.float64))
    i = int(np.argmax(ratio))
    print(f"gelu_erf_f: max |err| / |x| = {ratio[i]:.4e} at x = {float(x[nz][i])!r} (GELU_POLY = {GELU_POLY})")
    assert ratio[i] <= GELU_POLY
