"""fp64 restatement of UniPC (Zhao et al. 2023, "UniPC: A Unified Predictor-Corrector Framework for Fast Sampling of
Diffusion Models", Algorithms 5-8 in the multistep B(h) form that diffusers' UniPCMultistepScheduler runs) and of the Karras
sigma table (Karras et al. 2022, eq. 5), for the tests of ``UniPCScheduler`` and ``use_karras_sigmas``.

Written as step-by-step tensor arithmetic in float64 -- explicit ``D1s`` lists, a ``torch.linalg.solve`` per update, ``uni_c``
then ``uni_p``, ``model_outputs`` / ``last_sample`` state -- NOT from the product's coefficient rows.  The class takes its sigma
table as an argument, so a test can check the table and the step arithmetic separately.
"""
import math

import torch

from tests.sched_ref import F64, to_x0_eps


def asl(sigma):
    """(alpha_t, sigma_t, lambda_t) of a sigma: x_t = alpha_t x0 + sigma_t eps with alpha_t^2 + sigma_t^2 = 1."""
    a = 1.0 / math.sqrt(sigma * sigma + 1.0)
    s = sigma * a
    return a, s, (math.log(a) - math.log(s)) if s > 0 else math.inf


def _expm1(v):
    return math.expm1(v) if math.isfinite(v) else (-1.0 if v < 0 else math.inf)


class UniPC:
    """UniPCMultistepScheduler.step on a given sigma table (n + 1 entries): convert, correct the incoming sample with the new
    model output (uni_c), shift the history, choose the order, predict (uni_p).  ``step`` returns (prev, x0_pred) like the
    product, and keeps ``last_sample`` (the corrected sample) and ``m_t`` for the tests that look at them."""

    def __init__(self, sigmas, timesteps, pred="epsilon", solver_order=2, solver_type="bh2", predict_x0=True,
                 lower_order_final=True, disable_corrector=()):
        self.sig = [float(s) for s in sigmas]
        self.ts = list(timesteps)
        self.pred, self.order, self.type, self.px0 = pred, solver_order, solver_type, predict_x0
        self.lof, self.disabled = lower_order_final, set(disable_corrector)
        self.outs = [None] * solver_order
        self.last_sample, self.this_order, self.lower, self.i = None, 0, 0, None
        self.m_t = None

    def convert(self, m, x, i):
        a, s, _ = asl(self.sig[i])
        x0, eps = to_x0_eps(self.pred, m.to(F64), x.to(F64), a, s)
        return (x0 if self.px0 else eps), x0

    def _weights(self, h, rks, order):
        """(h_phi_1, B_h, R, b) of the paper's linear system R rho = b, built by the recurrence on phi_k."""
        hh = -h if self.px0 else h
        h_phi_1 = _expm1(hh)
        B_h = hh if self.type == "bh1" else _expm1(hh)
        h_phi_k = h_phi_1 / hh - 1.0
        fact = 1
        R, b = [], []
        rk = torch.tensor(rks, dtype=F64)
        for j in range(1, order + 1):
            R.append(rk ** (j - 1))
            b.append(h_phi_k * fact / B_h)
            fact *= j + 1
            h_phi_k = h_phi_k / hh - 1.0 / fact
        return h_phi_1, B_h, torch.stack(R), torch.tensor(b, dtype=F64)

    def uni_p(self, x, order):
        i = self.i
        m0 = self.outs[-1]
        a_t, s_t, l_t = asl(self.sig[i + 1])
        a_0, s_0, l_0 = asl(self.sig[i])
        h = l_t - l_0
        if not math.isfinite(h):                        # the step onto sigma 0: e^{-h} = 0, sigma_t = 0 (first order)
            assert order == 1
            if self.px0:
                return a_t * m0
            return (a_t / a_0) * x - (a_t * s_0 / a_0) * m0
        rks, D1s = [], []
        for k in range(1, order):
            mi = self.outs[-(k + 1)]
            rk = (asl(self.sig[i - k])[2] - l_0) / h
            rks.append(rk)
            D1s.append((mi - m0) / rk)
        rks.append(1.0)
        h_phi_1, B_h, R, b = self._weights(h, rks, order)
        if D1s:
            rhos = torch.tensor([0.5], dtype=F64) if order == 2 else torch.linalg.solve(R[:-1, :-1], b[:-1])
            res = sum(r.item() * d for r, d in zip(rhos, D1s))
        else:
            res = 0.0
        if self.px0:
            return (s_t / s_0) * x - a_t * h_phi_1 * m0 - a_t * B_h * res
        return (a_t / a_0) * x - s_t * h_phi_1 * m0 - s_t * B_h * res

    def uni_c(self, model_t, x_last, order):
        i = self.i
        m0 = self.outs[-1]                               # (before the shift: the previous step's entry)
        a_t, s_t, l_t = asl(self.sig[i])
        a_0, s_0, l_0 = asl(self.sig[i - 1])
        h = l_t - l_0
        rks, D1s = [], []
        for k in range(1, order):
            mi = self.outs[-(k + 1)]
            rk = (asl(self.sig[i - (k + 1)])[2] - l_0) / h
            rks.append(rk)
            D1s.append((mi - m0) / rk)
        rks.append(1.0)
        h_phi_1, B_h, R, b = self._weights(h, rks, order)
        rhos = torch.tensor([0.5], dtype=F64) if order == 1 else torch.linalg.solve(R, b)
        res = sum(r.item() * d for r, d in zip(rhos[:-1], D1s)) if D1s else 0.0
        D1_t = model_t - m0
        if self.px0:
            return (s_t / s_0) * x_last - a_t * h_phi_1 * m0 - a_t * B_h * (res + rhos[-1].item() * D1_t)
        return (a_t / a_0) * x_last - s_t * h_phi_1 * m0 - s_t * B_h * (res + rhos[-1].item() * D1_t)

    def step(self, m, t, x, **_):
        x = x.to(F64)
        if self.i is None:
            idx = [j for j, v in enumerate(self.ts) if v == int(t)]
            self.i = idx[1] if len(idx) > 1 else idx[0]
        i, n = self.i, len(self.ts)
        use_corrector = i > 0 and (i - 1) not in self.disabled and self.last_sample is not None
        m_t, x0 = self.convert(m, x, i)
        if use_corrector:
            x = self.uni_c(m_t, self.last_sample, self.this_order)
        self.outs = self.outs[1:] + [m_t]
        this_order = min(self.order, n - i) if self.lof else self.order
        self.this_order = min(this_order, self.lower + 1)
        self.last_sample = x
        self.m_t = m_t
        prev = self.uni_p(x, self.this_order)
        if self.lower < self.order:
            self.lower += 1
        self.i += 1
        return prev, x0


# ------------------------------------------------------------------------------------------------ Karras sigmas
def sigma_to_t(sigma, log_sigmas):
    """The training timestep of a sigma: linear interpolation in log sigma between the two table entries that bracket it
    (``log_sigmas``: float64, ascending in t), clamped to the table."""
    ls = math.log(max(sigma, 1e-10))
    n = log_sigmas.numel()
    low = 0
    for j in range(n):
        if ls >= log_sigmas[j].item():
            low = j
    low = min(low, n - 2)
    lo, hi = log_sigmas[low].item(), log_sigmas[low + 1].item()
    w = min(max((lo - ls) / (lo - hi), 0.0), 1.0)
    return (1.0 - w) * low + w * (low + 1)


def karras_table(ac, n, final_sigmas_type="zero", rho=7.0):
    """(timesteps, sigmas with the final sigma appended), float64, from an alpha-bar table: Karras et al. 2022 eq. 5 between
    sigma_max (t = T - 1) and sigma_min (t = 0); timestep_i = round(sigma_to_t(sigma_i))."""
    ac = ac.to(F64)
    train = ((1.0 - ac) / ac).sqrt()
    smax, smin = train[-1].item(), train[0].item()
    sig = []
    for j in range(n):
        ramp = j / (n - 1) if n > 1 else 0.0
        sig.append((smax ** (1.0 / rho) + ramp * (smin ** (1.0 / rho) - smax ** (1.0 / rho))) ** rho)
    log_sigmas = train.log()
    ts = [int(round(sigma_to_t(s, log_sigmas))) for s in sig]
    sig.append(smin if final_sigmas_type == "sigma_min" else 0.0)
    return ts, sig
