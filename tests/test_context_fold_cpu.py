"""The operator entry points of the prompt-side operand builders (tests/test_context_fold_gpu.py) are exported and bound, and the
slot permutation and tiling that file states once are what it takes them for.  No GPU needed."""
import torch

from sonicdiffusionbayeslab_amd import _lib
from tests.test_context_fold_gpu import perm16, retile32_ref, untile32

NEW_OPS = ("sd_op_xattn_expand", "sd_op_transpose_bf16", "sd_op_retile32", "sd_op_xattn_fold", "sd_op_ip_fold")


def test_fold_operator_symbols_are_exported_and_the_abi_version_stays(sdlib):
    declared = _lib.declared_symbols()
    for n in NEW_OPS:
        assert hasattr(sdlib, n), f"{n} is not exported"
        assert n in _lib._SIGS, f"{n} has no signature in _lib._SIGS"
        assert n in declared, f"{n} is not declared in include/sd_hip.h"
    assert sdlib.sd_abi_version() == 3


def test_perm16_is_an_involution_inside_every_group_of_16():
    r = torch.arange(1600)
    p = perm16(r)
    assert torch.equal(perm16(p), r)
    assert torch.equal(p // 16, r // 16) and torch.equal(torch.sort(p).values, r)
    assert torch.equal(p[:16], torch.tensor([0, 1, 2, 3, 8, 9, 10, 11, 4, 5, 6, 7, 12, 13, 14, 15]))


def test_untile32_inverts_retile32_ref():
    for B, R, K, RT in ((2, 640, 320, 640), (2, 320, 640, 32), (3, 64, 96, 16)):
        src = torch.arange(B * R * K, dtype=torch.int32).view(B, R, K)
        t = retile32_ref(src, B, R, K, RT)
        assert t.shape == (B, R // RT, K // 32, RT, 32)
        # element (row, col) sits at [row / RT][col / 32][row % RT][col % 32]
        assert int(t[B - 1, (R - 1) // RT, (K - 5) // 32, (R - 1) % RT, (K - 5) % 32]) == int(src[B - 1, R - 1, K - 5])
        assert torch.equal(untile32(t, B, R, K, RT), src)
