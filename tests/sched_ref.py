"""fp64 restatement of the v-prediction / sample conversions, the zero-terminal-SNR schedule and rescaled CFG, for the
tests of those features (the oracle's schedulers are epsilon-only).

Written from the published algorithms (diffusers 0.32.1's DDIMScheduler, DPMSolverMultistepScheduler, LCMScheduler,
PNDMScheduler and ``rescale_noise_cfg``; Lin et al. 2023, Algorithm 1) as step-by-step tensor arithmetic in float64,
NOT from the product's coefficient tables.  Each scheduler takes its alpha-bar table as an argument, so that a test can
check the table and the step arithmetic separately.
"""
import math

import torch

F64 = torch.float64


# ------------------------------------------------------------------------------------------------ schedules
def betas_fp32(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear"):
    """The fp32 betas every scheduler starts from (the input of the schedule, as upstream builds it)."""
    if beta_schedule == "scaled_linear":
        return torch.linspace(beta_start ** 0.5, beta_end ** 0.5, num_train_timesteps, dtype=torch.float32) ** 2
    return torch.linspace(beta_start, beta_end, num_train_timesteps, dtype=torch.float32)


def alphas_cumprod(betas, zero_snr=False):
    """alpha_bar in float64 from the given betas; ``zero_snr``: Lin et al. 2023, Algorithm 1 (sqrt(alpha_bar) shifted to
    end at exactly 0 and scaled to keep its first value)."""
    ab = torch.cumprod(1.0 - betas.to(F64), 0)
    if not zero_snr:
        return ab
    s = ab.sqrt()
    s0, sT = s[0].item(), s[-1].item()
    s = (s - sT) * (s0 / (s0 - sT))
    return s * s


def zero_snr_table_bound(betas):
    """A-priori bound on |alpha_bar_fp32 - alpha_bar| for the zero-SNR table computed in fp32 (cumprod of 1 - beta,
    sqrt, shift, scale, square, ratio, 1 - ratio, cumprod again).  Per index k, the fp32 cumprod carries a relative error
    <= (2k + 2) u; the shift subtracts sqrt(alpha_bar_T) (absolute error <= (k + T + 4) u sqrt(alpha_bar_0) after the
    sqrt and the subtraction); scale, square, ratio and the second cumprod add (2k + 8) u relative.  The bound is
    written in the sqrt domain (E_s, absolute) and mapped back: |d(s^2)| <= 2 s E_s + E_s^2, plus the relative term."""
    u = 2.0 ** -24
    ab0 = torch.cumprod(1.0 - betas.to(F64), 0)
    T = ab0.numel()
    k = torch.arange(T, dtype=F64)
    s = alphas_cumprod(betas, True).sqrt()
    es = (k + T + 8.0) * u * ab0[0].sqrt() * 2.0
    rel = (4.0 * k + 16.0) * u
    return 2.0 * s * es + es * es + rel * s * s + 2.0 ** -126


def dpm_sigmas(ac, timesteps, final_sigmas_type):
    """DPM-Solver's sigma table: sqrt((1 - ab) / ab) at the timesteps (integer timesteps: no interpolation), then the
    final sigma."""
    ac = ac.to(F64)
    sig = ((1.0 - ac) / ac).sqrt()
    out = [sig[int(t)].item() for t in timesteps]
    out.append(sig[0].item() if final_sigmas_type == "sigma_min" else 0.0)
    return out


# ------------------------------------------------------------------------------------------------ rescaled CFG
def cfg_combine(u, c, s):
    return u.to(F64) + s * (c.to(F64) - u.to(F64))


def rescale_factor(g, c, r):
    """k_b with rescale_noise_cfg(g, c, r) == k_b * g, torch.std semantics (unbiased), float64."""
    dims = list(range(1, g.dim()))
    std_c = c.to(F64).std(dim=dims, keepdim=True)
    std_g = g.to(F64).std(dim=dims, keepdim=True)
    return r * std_c / std_g + (1.0 - r)


def rescale_noise_cfg(g, c, r):
    """diffusers' rescale_noise_cfg (Lin et al. 2023, section 3.4), float64."""
    dims = list(range(1, g.dim()))
    g, c = g.to(F64), c.to(F64)
    std_c = c.std(dim=dims, keepdim=True)
    std_g = g.std(dim=dims, keepdim=True)
    return r * (g * (std_c / std_g)) + (1.0 - r) * g


def guided(e2, s, r):
    """[u | c] UNet output -> the prediction the step sees (CFG combine, then rescale when r > 0)."""
    u, c = e2.to(F64).chunk(2)
    g = cfg_combine(u, c, s)
    return rescale_noise_cfg(g, c, r) if r > 0.0 else g


# ------------------------------------------------------------------------------------------------ conversions
def to_x0_eps(pred, m, x, alpha, sigma):
    """(x0, eps) from a model output m at x = alpha x0 + sigma eps."""
    if pred == "epsilon":
        return (x - sigma * m) / alpha, m
    if pred == "v_prediction":
        return alpha * x - sigma * m, alpha * m + sigma * x
    if pred == "sample":
        return m, (x - alpha * m) / sigma
    raise ValueError(pred)


# ------------------------------------------------------------------------------------------------ schedulers
class DDIM:
    """DDIMScheduler.step, eta = 0: prev = sqrt(ab_prev) x0 + sqrt(1 - ab_prev) eps."""

    def __init__(self, ac, timesteps, pred, final_alpha_cumprod, T=1000):
        self.ac, self.ts, self.pred, self.final, self.T = ac.to(F64), list(timesteps), pred, final_alpha_cumprod, T

    def step(self, m, t, x, **_):
        m, x = m.to(F64), x.to(F64)
        prev_t = t - self.T // len(self.ts)
        a = self.ac[t].item()
        ap = self.ac[prev_t].item() if prev_t >= 0 else self.final
        x0, eps = to_x0_eps(self.pred, m, x, math.sqrt(a), math.sqrt(1.0 - a))
        return math.sqrt(ap) * x0 + math.sqrt(1.0 - ap) * eps, x0


class LCM:
    """LCMScheduler.step: boundary-condition scalings on x0, re-noised with ``noise`` on every step but the last."""

    def __init__(self, ac, timesteps, pred, final_alpha_cumprod, timestep_scaling=10.0):
        self.ac, self.ts, self.pred, self.final, self.scaling = ac.to(F64), list(timesteps), pred, final_alpha_cumprod, timestep_scaling
        self.i = 0

    def step(self, m, t, x, noise=None, **_):
        m, x = m.to(F64), x.to(F64)
        i = self.i
        prev_t = self.ts[i + 1] if i + 1 < len(self.ts) else t
        a = self.ac[t].item()
        ap = self.ac[prev_t].item() if prev_t >= 0 else self.final
        st = t * self.scaling
        c_skip = 0.25 / (st ** 2 + 0.25)
        c_out = st / (st ** 2 + 0.25) ** 0.5
        x0, _ = to_x0_eps(self.pred, m, x, math.sqrt(a), math.sqrt(1.0 - a))
        den = c_out * x0 + c_skip * x
        self.i += 1
        if i == len(self.ts) - 1:
            return den, den
        return math.sqrt(ap) * den + math.sqrt(1.0 - ap) * noise.to(F64), den


class PNDM:
    """PNDMScheduler.step_plms (skip_prk_steps): the PLMS combination of the raw model outputs, converted from v to eps
    inside _get_prev_sample with that call's alpha_bar and sample."""

    def __init__(self, ac, timesteps, num_inference_steps, pred, final_alpha_cumprod, T=1000):
        self.ac, self.ts, self.n, self.pred, self.final, self.T = ac.to(F64), list(timesteps), num_inference_steps, pred, final_alpha_cumprod, T
        self.ets, self.counter, self.cur = [], 0, None

    def _prev(self, x, t, prev_t, m):
        a = self.ac[t].item()
        ap = self.ac[prev_t].item() if prev_t >= 0 else self.final
        if self.pred == "v_prediction":
            m = a ** 0.5 * m + (1.0 - a) ** 0.5 * x
        sample_coeff = (ap / a) ** 0.5
        denom = a * (1.0 - ap) ** 0.5 + (a * (1.0 - a) * ap) ** 0.5
        return sample_coeff * x - (ap - a) * m / denom

    def step(self, m, t, x, **_):
        m, x = m.to(F64), x.to(F64)
        prev_t = t - self.T // self.n
        if self.counter != 1:
            self.ets = self.ets[-3:]
            self.ets.append(m)
        else:
            prev_t = t
            t = t + self.T // self.n
        e = self.ets
        if len(e) == 1 and self.counter == 0:
            mm = m
            self.cur = x
        elif len(e) == 1 and self.counter == 1:
            mm = (m + e[-1]) / 2
            x = self.cur
            self.cur = None
        elif len(e) == 2:
            mm = (3 * e[-1] - e[-2]) / 2
        elif len(e) == 3:
            mm = (23 * e[-1] - 16 * e[-2] + 5 * e[-3]) / 12
        else:
            mm = (1 / 24) * (55 * e[-1] - 59 * e[-2] + 37 * e[-3] - 9 * e[-4])
        self.counter += 1
        return (self._prev(x, t, prev_t, mm),)


class DPM:
    """DPMSolverMultistepScheduler (midpoint, orders 1-3, the four algorithm types) with the reference's step returning
    (prev, x0_pred)."""

    def __init__(self, ac, timesteps, pred, algorithm_type="dpmsolver++", solver_order=2, final_sigmas_type="zero",
                 lower_order_final=True, euler_at_final=False):
        self.ts = list(timesteps)
        self.sig = dpm_sigmas(ac, self.ts, final_sigmas_type)
        self.pred, self.alg, self.order, self.fst = pred, algorithm_type, solver_order, final_sigmas_type
        self.lof, self.eaf = lower_order_final, euler_at_final
        self.outs = [None] * solver_order
        self.lower = 0
        self.i = None

    def _asl(self, j):
        s = self.sig[j]
        a = 1.0 / math.sqrt(s * s + 1.0)
        sg = s * a
        return a, sg, (math.log(a) - math.log(sg)) if sg > 0 else math.inf

    def convert(self, m, x, i=None):
        i = (self.i if self.i is not None else 0) if i is None else i
        a, s, _ = self._asl(i)
        x0, eps = to_x0_eps(self.pred, m.to(F64), x.to(F64), a, s)
        if self.alg in ("dpmsolver++", "sde-dpmsolver++"):
            return x0, x0
        return eps, (x.to(F64) - s * eps) / a

    def push(self, m, x):
        """The variant pipelines' history hand-off: convert at the current index, shift, append."""
        out, _ = self.convert(m, x)
        self.outs = self.outs[1:] + [out]

    def step(self, m, t, x, variance_noise=None, **_):
        x = x.to(F64)
        if self.i is None:
            idx = [j for j, v in enumerate(self.ts) if v == int(t)]
            self.i = idx[1] if len(idx) > 1 else idx[0]
        i, n = self.i, len(self.ts)
        lof = (i == n - 1) and (self.eaf or (self.lof and n < 15) or self.fst == "zero")
        los = (i == n - 2) and self.lof and n < 15
        out, x0 = self.convert(m, x, i)
        self.outs = self.outs[1:] + [out]
        if self.order == 1 or self.lower < 1 or lof:
            k = 1
        elif self.order == 2 or self.lower < 2 or los:
            k = 2
        else:
            k = 3
        z = variance_noise.to(F64) if variance_noise is not None else None
        at, st, lt = self._asl(i + 1)
        a0, s0, l0 = self._asl(i)
        h = lt - l0
        E = lambda v: math.exp(v) if math.isfinite(v) else (0.0 if v < 0 else math.inf)
        m0 = self.outs[-1]
        if k == 1:
            D = [m0]
        elif k == 2:
            _, _, l1 = self._asl(i - 1)
            r0 = (l0 - l1) / h
            D = [m0, (1.0 / r0) * (m0 - self.outs[-2])]
        else:
            _, _, l1 = self._asl(i - 1)
            _, _, l2 = self._asl(i - 2)
            r0, r1 = (l0 - l1) / h, (l1 - l2) / h
            d10 = (1.0 / r0) * (m0 - self.outs[-2])
            d11 = (1.0 / r1) * (self.outs[-2] - self.outs[-3])
            D = [m0, d10 + (r0 / (r0 + r1)) * (d10 - d11), (1.0 / (r0 + r1)) * (d10 - d11)]
        if self.alg == "dpmsolver++":
            y = (st / s0) * x - at * (E(-h) - 1.0) * D[0]
            if k == 2:
                y = y - 0.5 * at * (E(-h) - 1.0) * D[1]
            elif k == 3:
                y = y + at * ((E(-h) - 1.0) / h + 1.0) * D[1] - at * ((E(-h) - 1.0 + h) / h ** 2 - 0.5) * D[2]
        elif self.alg == "dpmsolver":
            y = (at / a0) * x - st * (E(h) - 1.0) * D[0]
            if k == 2:
                y = y - 0.5 * st * (E(h) - 1.0) * D[1]
            elif k == 3:
                y = y - st * ((E(h) - 1.0) / h - 1.0) * D[1] - st * ((E(h) - 1.0 - h) / h ** 2 - 0.5) * D[2]
        elif self.alg == "sde-dpmsolver++":
            q = 1.0 - E(-2.0 * h)
            y = (st / s0 * E(-h)) * x + at * q * D[0] + st * math.sqrt(q) * z
            if k == 2:
                y = y + 0.5 * at * q * D[1]
            elif k == 3:
                y = y + at * (q / (-2.0 * h) + 1.0) * D[1] + at * ((q - 2.0 * h) / (2.0 * h) ** 2 - 0.5) * D[2]
        else:                                                   # sde-dpmsolver (orders 1 and 2)
            y = (at / a0) * x - 2.0 * st * (E(h) - 1.0) * D[0] + st * math.sqrt(E(2.0 * h) - 1.0) * z
            if k == 2:
                y = y - st * (E(h) - 1.0) * D[1]
            assert k < 3
        if self.lower < self.order:
            self.lower += 1
        self.i += 1
        return y, x0


# ------------------------------------------------------------------------------------------------ test drivers
# (pairs a product scheduler with its restatement; shared by the CPU and GPU tests)
NAMES = {"ddim": "ddim_scheduler", "dpm": "dpm_solver_scheduler", "lcm": "lcm_scheduler", "pndm": "pndm_scheduler"}


def make_pair(kind, n, pred, zero_snr=False, **kw):
    """(product scheduler after set_timesteps(n), fp64 restatement on the product's own alpha-bar table)."""
    from sonicdiffusionbayeslab_amd.registry import schedulers_registry
    from sonicdiffusionbayeslab_amd.schedulers import PNDMConfigStub
    s = schedulers_registry[NAMES[kind]].from_config(PNDMConfigStub().config, prediction_type=pred,
                                                     rescale_betas_zero_snr=zero_snr, **kw)
    s.set_timesteps(n)
    ac = torch.from_numpy(s.alphas_cumprod).to(F64)
    ts = list(s._timesteps_list)
    if kind == "ddim":
        ref = DDIM(ac, ts, pred, s.final_alpha_cumprod)
    elif kind == "lcm":
        ref = LCM(ac, ts, pred, s.final_alpha_cumprod)
    elif kind == "pndm":
        ref = PNDM(ac, ts, n, pred, s.final_alpha_cumprod)
    else:
        c = s.config
        ref = DPM(ac, ts, pred, c.algorithm_type, c.solver_order, c.final_sigmas_type, c.lower_order_final,
                  c.euler_at_final)
    return s, ref


def run_teacher_forced(s, ref, kind, shape, guidance, rescale, device, check, seed=5):
    """Every step of the schedule on random [u | c] model outputs: the product's step_fused (CFG + rescale inside) and the
    restatement (fp64 combine + rescale_noise_cfg + step) from the same fp32 sample; the next step starts from the
    restatement's result.  ``check(i, product_outputs, reference_outputs)``."""
    g = torch.Generator().manual_seed(seed)
    B = shape[0]
    x = torch.randn(shape, generator=g)
    sde = kind == "dpm" and s.config.algorithm_type.startswith("sde-")
    for i, t in enumerate(list(s._timesteps_list)):
        e2 = torch.randn((2 * B,) + tuple(shape[1:]), generator=g)
        kwo, kws = {}, {}
        if kind == "lcm" and i < len(s._timesteps_list) - 1:
            z = torch.randn(shape, generator=g)
            kwo["noise"], kws["noise"] = z, z.to(device)
        if sde:
            z = torch.randn(shape, generator=g)
            kwo["variance_noise"], kws["variance_noise"] = z, z.to(device)
        want = ref.step(guided(e2, guidance, rescale), t, x, **kwo)
        got = s.step_fused(e2.to(device), guidance, x.to(device), t, cfg=True, guidance_rescale=rescale, **kws)
        assert len(got) == len(want)
        check(i, got, want)
        x = want[0].float()
