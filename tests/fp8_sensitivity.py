"""How far the fp8 emulating oracle moves under a tiny perturbation of its own quantised tensors -- the reference's own
sensitivity, from which the model-level fp8 gates and the calibration check take their bounds (tests/test_fp8_gpu.py), and
the test-side mirror of ``sd_unet_calibrate_fp8``.  Pure PyTorch on the CPU; the constants below are pinned to within 10 %
by tests/test_fp8_sensitivity_cpu.py, which recomputes them.

Measured on the seeded 16x16 UNet (weights seed 1234, inputs seed 29) at t = 499, rel-L2 of the emulating oracle's output:

    checkpoint                        scheme (vs the unquantised oracle)   x (1 + d), |d| <= 2^-23    |d| <= 2^-8
    ordinary (default scales 8 / 2)   0.0950                               0.0540, 0.0545             0.0758, 0.0771
    30x gains (calibrated scales)     0.1603                               0.0766, 0.0975             0.1422, 0.1442

(perturbation seeds 0 and 1; SCHEME / D23 / D8 below hold the seed-0 column.)

The perturbation multiplies every tensor entering ``act_norm`` / ``act_ff`` by (1 + d), d uniform in +-amplitude, before it
is rounded.  Even one fp32 ulp (2^-23) moves the output by about half the scheme's own distance from the unquantised
oracle: e4m3 rounding turns any difference into noise of the scheme's own size within a few layers.  Two correct
implementations of the scheme therefore agree only to about D8 at forward level, and a forward-level gate says almost
nothing about one GroupNorm kernel: the fp8 path is pinned at operator level (flip budgets, amax) and at calibration.
"""
import math

import numpy as np
import torch

from oracle.fp8 import E4M3_MAX, Fp8Emulation, e4m3_round

T_SENS = 499.0
MARGIN = 2.0
HOT_GAIN = 30.0

# rel-L2 at t = 499 (tests/test_fp8_sensitivity_cpu.py recomputes each and pins it to within 10 %)
SCHEME = {"ordinary": 9.50e-2, "hot": 1.603e-1}
D23 = {"ordinary": 5.40e-2, "hot": 7.66e-2}
D8 = {"ordinary": 7.58e-2, "hot": 1.422e-1}


def product_scale(amax, margin=MARGIN):
    """The rule of sd_unet_calibrate_fp8 (csrc/unet.hip), in its fp32 arithmetic: the largest power of two
    <= 448 / (margin amax), inside 2^-20 .. 2^20."""
    want = np.float32(448.0) / (np.float32(margin) * max(np.float32(amax), np.float32(1e-6)))
    e = math.frexp(float(want))[1] - 1                      # floor(log2(want)), exact
    return float(min(max(2.0 ** e, 2.0 ** -20), 2.0 ** 20))


class PerturbedEmulation(Fp8Emulation):
    """Fp8Emulation whose quantised tensors are multiplied by (1 + d), d uniform in +-amp, before they are rounded."""

    def __init__(self, weights, amp=0.0, seed=0, share=None, **kw):
        """``share``: an Fp8Emulation of the same weights whose quantised weights are reused (quantising them again costs
        as much as a forward)."""
        super().__init__({} if share is not None else weights, **kw)
        if share is not None:
            self.wq = share.wq
        self.amp = float(amp)
        self.gen = torch.Generator().manual_seed(seed)

    def _perturb(self, x):
        if self.amp == 0.0:
            return x
        d = (torch.rand(x.shape, generator=self.gen, dtype=torch.float64) * 2.0 - 1.0) * self.amp
        return (x.double() * (1.0 + d)).float()

    def act_norm(self, x, name=None):
        return super().act_norm(self._perturb(x), name)

    def act_ff(self, x, name=None):
        return super().act_ff(self._perturb(x), name)


class CalibratingEmulation(PerturbedEmulation):
    """The mirror of sd_unet_calibrate_fp8: every e4m3 activation tensor records its amax (accumulated over the forwards
    run through this object), takes the product's scale for it and is rounded with that scale before the forward goes on
    -- Fp8AmaxRecorder passes the activations unrounded, the product does not."""

    def __init__(self, weights, margin=MARGIN, amp=0.0, seed=0, share=None):
        super().__init__(weights, amp=amp, seed=seed, share=share)
        self.margin = float(margin)
        self.amax = {}

    def _calibrated(self, x, name):
        x = self._perturb(x)
        self.amax[name] = max(self.amax.get(name, 0.0), float(x.abs().max()))
        s = self.scales[name] = product_scale(self.amax[name], self.margin)
        return e4m3_round(x * s) / s

    def act_norm(self, x, name=None):
        return self._calibrated(x, name)

    def act_ff(self, x, name=None):
        return self._calibrated(x, name)


def hot_keys(sd):
    return [k for k in sd if k.endswith(("resnets.0.norm2.weight", "transformer_blocks.0.norm3.weight")) and "down_blocks.1" in k]


def checkpoint(sd, which):
    """"ordinary": the seeded synthetic weights; "hot": two norm gains of down block 1 times 30 (real SD-1.5 has such
    layers), as tests/test_fp8_gpu.py::test_fp8_calibration_positions_the_range builds it."""
    if which == "ordinary":
        return sd
    out = dict(sd)
    for k in hot_keys(sd):
        out[k] = (sd[k] * HOT_GAIN).to(torch.bfloat16).float()
    return out


def damax(ref, other):
    """The largest relative amax difference over the tensors of two calibrations (the same names on both sides)."""
    assert set(ref) == set(other)
    return max(abs(other[k] / ref[k] - 1.0) for k in ref)
