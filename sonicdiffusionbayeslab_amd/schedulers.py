"""The reference's three scheduler plugins, with ``step`` as ONE fused HIP launch.

Same registry keys, class names and call protocol as ``src/schedulers.py`` of the reference:

* ``"dpm_solver_scheduler"`` -> ``DPMSolverScheduler``  (``src/schedulers.py:12-187``)
* ``"ddim_scheduler"``       -> ``DDIMSchedulerMy``     (``src/schedulers.py:190-192``)
* ``"lcm_scheduler"``        -> ``LCMScheduler``        (``src/schedulers.py:195-197``)
* ``"pndm_scheduler"``       -> ``PNDMScheduler``       (the checkpoint's own scheduler)
* ``"unipc_scheduler"``      -> ``UniPCScheduler``      (diffusers' UniPCMultistepScheduler; its step is ``sd_sched_step_pc``)

Protocol kept: ``from_config(config, **overrides)``, ``.config``, ``.order``,
``.init_noise_sigma``, ``set_timesteps(n, device=)``, ``.timesteps``, ``scale_model_input``,
``step(model_output, timestep, sample, ..., return_dict=False) -> (prev_sample, x0_pred)``,
and for DPM ``convert_model_output`` / ``.model_outputs``.

MI355X-first design: the host keeps the fp32 alpha-bar / sigma tables exactly as diffusers builds
them, derives the step's scalar coefficients in fp64, and launches ``sd_sched_step`` once: CFG
combine + x0 + multistep update + history write in a single elementwise kernel with no host sync
(the reference does ~10 elementwise launches and an ``alphas_cumprod[t]`` device->host sync per
step).  ``step_fused`` is the loop's entry point (takes the raw 2B-batch UNet output and the
guidance scale); ``step`` is the drop-in signature and uses the same kernel without CFG.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import List, Optional

import numpy as np
import torch

from . import _lib
from . import dist as sdist
from .registry import schedulers_registry

# runwayml/stable-diffusion-v1-5 scheduler/scheduler_config.json (PNDM) + the defaults PNDM stores;
# this is what ``from_config(self.model.scheduler.config)`` receives
# (src/experiments/base_experiment.py:66-72).
SD15_SCHEDULER_CONFIG = dict(
    num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear",
    trained_betas=None, skip_prk_steps=True, set_alpha_to_one=False, prediction_type="epsilon",
    timestep_spacing="leading", steps_offset=1, clip_sample=False,
)


class SchedulerConfig(dict):
    """dict with attribute access (diffusers FrozenDict behaviour the reference relies on)."""

    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError:
            raise AttributeError(k) from None


def rescale_zero_terminal_snr(betas: torch.Tensor) -> torch.Tensor:
    """diffusers' ``rescale_zero_terminal_snr`` (Lin et al. 2023, Algorithm 1), in the same fp32 torch operations and
    order, so the tables are bit-identical to upstream's: shift sqrt(alpha_bar) to end at 0, rescale it to keep its
    first value, and return the betas of that schedule."""
    alphas_cumprod = torch.cumprod(1.0 - betas, dim=0)
    alphas_bar_sqrt = alphas_cumprod.sqrt()
    alphas_bar_sqrt_0 = alphas_bar_sqrt[0].clone()
    alphas_bar_sqrt_T = alphas_bar_sqrt[-1].clone()
    alphas_bar_sqrt -= alphas_bar_sqrt_T
    alphas_bar_sqrt *= alphas_bar_sqrt_0 / (alphas_bar_sqrt_0 - alphas_bar_sqrt_T)
    alphas_bar = alphas_bar_sqrt ** 2
    alphas = alphas_bar[1:] / alphas_bar[:-1]
    alphas = torch.cat([alphas_bar[0:1], alphas])
    return 1 - alphas


def _alphas_cumprod_fp32(cfg) -> np.ndarray:
    if cfg.get("trained_betas") is not None:
        betas = torch.tensor(cfg["trained_betas"], dtype=torch.float32)
    elif cfg["beta_schedule"] == "scaled_linear":
        betas = torch.linspace(cfg["beta_start"] ** 0.5, cfg["beta_end"] ** 0.5, cfg["num_train_timesteps"],
                               dtype=torch.float32) ** 2
    elif cfg["beta_schedule"] == "linear":
        betas = torch.linspace(cfg["beta_start"], cfg["beta_end"], cfg["num_train_timesteps"], dtype=torch.float32)
    else:
        raise NotImplementedError(f"beta_schedule {cfg['beta_schedule']}")
    if cfg.get("rescale_betas_zero_snr", False):
        betas = rescale_zero_terminal_snr(betas)
    return torch.cumprod(1.0 - betas, dim=0).numpy()


PREDICTION_TYPES = ("epsilon", "v_prediction", "sample")


def prediction_coefs(prediction_type: str, alpha: float, sigma: float):
    """(dx, de, ex, ee): x0 = dx*x + de*m and eps = ex*x + ee*m for a model output m at a step with x = alpha*x0 +
    sigma*eps (diffusers 0.32.1's conversions; alpha = sqrt(alpha_bar), sigma = sqrt(1 - alpha_bar) for DDIM / LCM / PNDM,
    DPM-Solver's alpha_t, sigma_t from its sigmas).  Every case is linear in (x, m), so each is a coefficient table of the
    one fused step."""
    if prediction_type == "epsilon":
        return 1.0 / alpha, -sigma / alpha, 0.0, 1.0
    if prediction_type == "v_prediction":
        return alpha, -sigma, sigma, alpha
    if prediction_type == "sample":
        return 0.0, 1.0, 1.0 / sigma, -alpha / sigma
    raise NotImplementedError(f"prediction_type {prediction_type!r}: {PREDICTION_TYPES} are built")


GUIDE_CFG_PAG, GUIDE_PAG = 2, 3       # include/sd_hip.h::SD_GUIDE_CFG_PAG / SD_GUIDE_PAG
GUIDE_CFG_SAG, GUIDE_SAG = 4, 5       # include/sd_hip.h::SD_GUIDE_CFG_SAG / SD_GUIDE_SAG
PRED_TYPE_IDS = {"epsilon": 0, "v_prediction": 1, "sample": 2}        # the pred_type of sd_op_sag_degrade


def sag_degrade_coef(prediction_type: str, alpha_prod_t: float):
    """The six fp32 coefficients of ``sd_op_sag_degrade`` for a step at ``alphas_cumprod[t] = alpha_prod_t``, derived in
    fp64: (x0 <- x, x0 <- m, eps <- x, eps <- m, sqrt(a), sqrt(1 - a)) with m the model output."""
    a = float(alpha_prod_t)
    sa, s1 = math.sqrt(a), math.sqrt(1.0 - a)
    if prediction_type == "epsilon":
        return (1.0 / sa, -s1 / sa, 0.0, 1.0, sa, s1)
    if prediction_type == "v_prediction":
        return (sa, -s1, s1, sa, sa, s1)
    if prediction_type == "sample":
        return (0.0, 1.0, 1.0 / s1, -sa / s1, sa, s1)
    raise NotImplementedError(f"prediction_type {prediction_type!r}: {PREDICTION_TYPES} are built")


def sag_degrade(x: torch.Tensor, m: torch.Tensor, mass: torch.Tensor, mh: int, mw: int, prediction_type: str, alpha_prod_t: float,
                out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``sd_op_sag_degrade``: the degraded, re-noised latents of a SAG step from the latents ``x`` [LB,4,H,W], the model output
    ``m`` on them and the attention masses ``mass`` [>= LB, mh * mw] (all fp32, contiguous, on one device)."""
    lib = _lib.load()
    if out is None:
        out = torch.empty_like(x)
    coef = (C.c_float * 6)(*sag_degrade_coef(prediction_type, alpha_prod_t))
    _lib.check(lib.sd_op_sag_degrade(_lib.current_stream(), x.data_ptr(), m.data_ptr(), mass.data_ptr(), int(mh), int(mw),
                                     PRED_TYPE_IDS[prediction_type], coef, out.data_ptr(), x.shape[0], x.shape[2], x.shape[3]),
               "sd_op_sag_degrade")
    return out


def pag_step_scale(pag_scale: float, pag_adaptive_scale: float, timestep) -> float:
    """The PAG scale of the step at ``timestep`` (diffusers' ``PAGMixin._get_pag_scale``): ``pag_scale`` when
    ``pag_adaptive_scale == 0``, else ``max(pag_scale - pag_adaptive_scale * (1000 - t), 0)``."""
    if pag_adaptive_scale == 0:
        return float(pag_scale)
    return max(float(pag_scale) - float(pag_adaptive_scale) * (1000.0 - float(timestep)), 0.0)


def cfg_rescale_factors(eps: torch.Tensor, batch: int, guidance: float, rescale: float, pag=None) -> torch.Tensor:
    """``sd_cfg_rescale_factors``: k[b] = rescale * std(c_b) / std(g_b) + (1 - rescale), g = u + guidance*(c - u), for
    eps = [u | c] (2*batch samples, fp32, contiguous).  diffusers' rescale_noise_cfg is g := k[b] * g.  ``pag`` (a PAG step
    scale): eps = [u | c | p] and g carries the PAG term, + pag*(c - p) (``sd_cfg_rescale_factors_pag``)."""
    lib = _lib.load()
    n = eps.numel() // ((2 if pag is None else 3) * batch)
    k = torch.empty(batch, dtype=torch.float32, device=eps.device)
    if pag is not None:
        _lib.check(lib.sd_cfg_rescale_factors_pag(_lib.current_stream(), eps.data_ptr(), int(batch), int(n), float(guidance),
                                                  float(pag), float(rescale), k.data_ptr()), "sd_cfg_rescale_factors_pag")
        return k
    _lib.check(lib.sd_cfg_rescale_factors(_lib.current_stream(), eps.data_ptr(), int(batch), int(n), float(guidance),
                                          float(rescale), k.data_ptr()), "sd_cfg_rescale_factors")
    return k


class _FusedStepScheduler:
    order = 1
    init_noise_sigma = 1.0
    _own_defaults: dict = {}
    _accepted: tuple = ()

    def __init__(self, **kwargs):
        cfg = dict(self._own_defaults)
        cfg.update(kwargs)
        self.config = SchedulerConfig(cfg)
        self.alphas_cumprod = _alphas_cumprod_fp32(self.config)      # fp32 table, as upstream
        if "set_alpha_to_one" in self.config:                        # (DDIM, LCM, PNDM: alpha_bar before the first timestep)
            self.final_alpha_cumprod = 1.0 if self.config.set_alpha_to_one else float(self.alphas_cumprod[0])
        self.timesteps: Optional[torch.Tensor] = None
        self.num_inference_steps: Optional[int] = None
        self._timesteps_list: List[int] = []
        self._step_index: Optional[int] = None

    # diffusers ConfigMixin.from_config: keep the keys this class accepts, apply overrides
    @classmethod
    def from_config(cls, config, **overrides):
        merged = dict(config)
        merged.update(overrides)
        return cls(**{k: v for k, v in merged.items() if k in cls._accepted})

    @property
    def step_index(self):
        return self._step_index

    def scale_model_input(self, sample, timestep=None):
        return sample

    def _set(self, ts: np.ndarray, device=None):
        self._timesteps_list = [int(t) for t in ts]
        self.timesteps = torch.from_numpy(np.asarray(ts, dtype=np.int64)).to(device) if device is not None \
            else torch.from_numpy(np.asarray(ts, dtype=np.int64))
        self.num_inference_steps = len(ts)
        self._step_index = None

    def _index_of(self, timestep) -> int:
        t = int(timestep)
        idx = [i for i, v in enumerate(self._timesteps_list) if v == t]
        if not idx:
            raise ValueError(f"timestep {t} is not in the schedule")
        return idx[1] if len(idx) > 1 else idx[0]

    # --- the single fused launch ------------------------------------------------------------
    @staticmethod
    def _launch(eps, cfg, guidance, x, m1, m2, noise, coef, want_y2=True, want_m=False, m3=None, k=None, blend=None, pag=None, sag=None):
        """coef = (px, pe, p1, p2, pn, yx, ye, mx, me[, p3]) -- see include/sd_hip.h::sd_sched_step.  ``k`` (per-sample
        rescaled-CFG factors, ``cfg_rescale_factors``): the step scales the combined prediction by them
        (sd_sched_step_rescaled); None launches sd_sched_step.  ``blend`` = (init, blend_noise, mask, a, s), the latent
        blend of inpainting (``_blend``): the same step as sd_sched_step_inpaint, with or without ``k`` -- still one launch.
        ``pag`` (the step's PAG scale): eps = [u | c | p] under ``cfg``, else [c | p], and the prediction carries the PAG
        term (sd_sched_step_pag, which takes ``k`` and ``blend`` as they come).  ``sag`` (the SAG scale): eps = [u | c | d]
        under ``cfg``, else [c | d], d the prediction on the degraded latents (sd_sched_step_sag, same operands)."""
        lib = _lib.load()
        n = x.numel()
        prev = torch.empty_like(x)
        y2 = torch.empty_like(x) if want_y2 else None
        mo = torch.empty_like(x) if want_m else None
        c10 = [float(v) for v in coef] + [0.0] * (10 - len(coef))
        head = (_lib.current_stream(), eps.data_ptr(), int(cfg), float(guidance), x.data_ptr(), _lib.ptr(m1), _lib.ptr(m2),
                _lib.ptr(m3), _lib.ptr(noise), prev.data_ptr(), _lib.ptr(y2), _lib.ptr(mo), (C.c_float * 10)(*c10), n)
        if pag is not None or sag is not None:
            init, bnoise, mask, a, s = blend if blend is not None else (None, None, None, 1.0, 0.0)
            if sag is not None:
                head = (*head[:2], GUIDE_CFG_SAG if cfg else GUIDE_SAG, float(guidance), float(sag), *head[4:])
            else:
                head = (*head[:2], GUIDE_CFG_PAG if cfg else GUIDE_PAG, float(guidance), float(pag), *head[4:])
            name, tail = "sd_sched_step_sag" if sag is not None else "sd_sched_step_pag", (_lib.ptr(k), n // x.shape[0], _lib.ptr(init), _lib.ptr(bnoise), _lib.ptr(mask),
                                               float(a), float(s), mask.numel() // mask.shape[0] if mask is not None else 0)
        elif blend is not None:
            init, bnoise, mask, a, s = blend
            name, tail = "sd_sched_step_inpaint", (_lib.ptr(k), n // x.shape[0], init.data_ptr(), bnoise.data_ptr(),
                                                   mask.data_ptr(), float(a), float(s), mask.numel() // mask.shape[0])
        elif k is not None:
            name, tail = "sd_sched_step_rescaled", (k.data_ptr(), n // x.shape[0])
        else:
            name, tail = "sd_sched_step", ()
        _lib.check(getattr(lib, name)(*head, *tail), name)
        return prev, y2, mo

    def _rescale(self, eps, cfg, guidance, guidance_rescale, x, pag=None, sag=None):
        """The rescaled-CFG factors of this step (``src/models.py:244-250``: only with CFG and guidance_rescale > 0),
        kept in ``rescale_factors`` for the variant pipelines' history hand-off; None otherwise.  ``pag``: the step's PAG
        scale -- the factors then describe the prediction with its PAG term."""
        self.rescale_factors = None
        self._pag_kw(pag, sag, guidance_rescale)        # (a SAG step refuses guidance_rescale before anything is launched)
        if cfg and guidance_rescale > 0.0:
            kw = {} if pag is None else {"pag": pag}        # (a plain step calls it as ever)
            self.rescale_factors = cfg_rescale_factors(eps, x.shape[0], guidance, guidance_rescale, **kw)
        return self.rescale_factors

    @staticmethod
    def _pag_kw(pag_scale, sag_scale=None, guidance_rescale=0.0):
        """The extra guidance branch of a step: ``pag=`` of ``_launch`` for a PAG step, ``sag=`` for a SAG step; nothing otherwise
        (as ``_blend_kw``).  A SAG step has no ``guidance_rescale`` (upstream's SAG pipeline has none, and the factors would be
        taken over a buffer with a third block) and no PAG term: refused by name before the step's launch."""
        if sag_scale is not None:
            if pag_scale is not None:
                raise NotImplementedError("a step with PAG and SAG together is not built")
            if guidance_rescale is not None and guidance_rescale > 0.0:
                raise NotImplementedError("a SAG step with guidance_rescale > 0 is not built (upstream's SAG pipeline has no rescale)")
            return {"sag": float(sag_scale)}
        return {} if pag_scale is None else {"pag": float(pag_scale)}

    def _check_prediction_type(self):
        if self.config.prediction_type not in PREDICTION_TYPES:
            raise NotImplementedError(f"prediction_type {self.config.prediction_type!r} is not built for "
                                      f"{type(self).__name__} (built: {PREDICTION_TYPES})")

    def _refuse_epsilon_at_zero_snr(self, ts, floor: float = 0.0):
        """Deliberate deviation from upstream: epsilon prediction at a step whose alpha_bar is 0 (a zero-terminal-SNR
        schedule reaching its last training timestep) divides by zero there, and upstream returns NaN latents.  This
        refuses the combination before any GPU work.  ``floor``: the value a scheduler has put in place of that 0
        (UniPC's 2^-24), which is refused like the 0 it stands for."""
        if self.config.prediction_type != "epsilon":
            return
        for t in ts:
            if float(self.alphas_cumprod[int(t)]) <= floor:
                raise ValueError(f"prediction_type='epsilon' with rescale_betas_zero_snr=True and timestep_spacing="
                                 f"{self.config.get('timestep_spacing')!r}: alpha_bar is 0 at timestep {int(t)}, where an "
                                 "epsilon prediction determines no x0; use prediction_type='v_prediction' (or 'sample')")

    @staticmethod
    def _prep(t: torch.Tensor) -> torch.Tensor:
        if not t.is_cuda:
            raise _lib.SdHipError("scheduler.step runs as a HIP kernel: tensors must live on the GPU")
        return t if (t.dtype == torch.float32 and t.is_contiguous()) else t.float().contiguous()

    rescale_factors: Optional[torch.Tensor] = None

    def _blend_kw(self, inpaint, x):
        """``blend=`` of ``_launch`` for an inpainting step; nothing otherwise: a CPU stand-in for ``_launch`` that knows no
        blend (tests/test_prediction_cpu.py) is then called as before."""
        return {} if inpaint is None else {"blend": self._blend(inpaint, x)}

    def _blend(self, inpaint, x):
        """``inpaint`` of ``step_fused`` -> the blend operands of the launch.  ``inpaint = (init, noise, mask,
        next_timestep_or_None)``: after the step, latents := mask ? prev : add_noise(init, noise, next_timestep), and ``init``
        itself after the last step (None).  ``init`` / ``noise``: fp32 like the sample; ``mask``: [B, 1, h, w] fp32 0 / 1.
        (a, s) are ``_add_noise_coefs`` of the next timestep, (1, 0) after the last step."""
        if inpaint is None:
            return None
        init, noise, mask, t_next = inpaint
        init, noise, mask = self._prep(init), self._prep(noise), self._prep(mask)
        if init.shape != x.shape or noise.shape != x.shape:
            raise ValueError(f"inpaint: init {tuple(init.shape)} / noise {tuple(noise.shape)} do not match the sample {tuple(x.shape)}")
        if mask.dim() != 4 or mask.shape[0] != x.shape[0] or mask.shape[1] != 1 or mask.shape[2:] != x.shape[2:]:
            raise ValueError(f"inpaint: mask {tuple(mask.shape)} must be [{x.shape[0]}, 1, {x.shape[2]}, {x.shape[3]}]")
        a, s = (1.0, 0.0) if t_next is None else self._add_noise_coefs(t_next)
        return init, noise, mask, a, s

    # --- forward process (image-to-image start; diffusers' ``add_noise``, upstream-recall) -----------------------------
    def _add_noise_coefs(self, timestep):
        """(sqrt(alpha_bar_t), sqrt(1 - alpha_bar_t)) from the fp32 table, as DDIM / LCM upstream."""
        a = float(self.alphas_cumprod[int(timestep)])
        return math.sqrt(a), math.sqrt(1.0 - a)

    def add_noise(self, original_samples, noise, timestep):
        """``sqrt(alpha_bar_t) * x0 + sqrt(1 - alpha_bar_t) * noise`` at one scalar ``timestep`` of the schedule, as ONE
        ``sd_sched_step`` launch (coef[0] on the sample, coef[4] on the noise operand; the prediction operand has
        coefficient 0).  Does not touch the multistep state."""
        if self.num_inference_steps is None:
            raise ValueError("run set_timesteps first")
        alpha, sigma = self._add_noise_coefs(timestep)
        x = self._prep(original_samples)
        z = self._prep(noise.to(x.device))
        if z.shape != x.shape:
            raise ValueError(f"add_noise: noise {tuple(z.shape)} does not match the samples {tuple(x.shape)}")
        noisy, _, _ = self._launch(x, False, 0.0, x, None, None, z, (alpha, 0, 0, 0, sigma, 0, 0, 0, 0), want_y2=False)
        return noisy

    def step(self, model_output, timestep, sample, eta: float = 0.0, generator=None, variance_noise=None,
             return_dict: bool = False, **kwargs):
        """Drop-in ``scheduler.step`` (CFG already combined by the caller, src/models.py:253)."""
        out_dtype = model_output.dtype
        kw = {"variance_noise": variance_noise} if variance_noise is not None else {}
        prev, x0 = self.step_fused(model_output, 0.0, sample, timestep, cfg=False, eta=eta, generator=generator, **kw)
        return (prev.to(out_dtype), x0.to(out_dtype))


@schedulers_registry.add_to_registry("ddim_scheduler")
class DDIMSchedulerMy(_FusedStepScheduler):
    """diffusers ``DDIMScheduler`` (eta = 0 path; the reference never passes another eta,
    ``src/models.py:43,185``).  A.6.1."""
    _own_defaults = dict(num_train_timesteps=1000, beta_start=0.0001, beta_end=0.02, beta_schedule="linear",
                         trained_betas=None, clip_sample=True, set_alpha_to_one=True, steps_offset=0,
                         prediction_type="epsilon", thresholding=False, timestep_spacing="leading",
                         rescale_betas_zero_snr=False)
    _accepted = tuple(_own_defaults)

    def __init__(self, **kwargs):
        super().__init__(**kwargs)
        if self.config.clip_sample or self.config.thresholding:
            raise NotImplementedError("clip_sample / thresholding are not on the hot path")
        self._check_prediction_type()

    def set_timesteps(self, num_inference_steps: int, device=None):
        T = self.config.num_train_timesteps
        if num_inference_steps > T:
            raise ValueError("num_inference_steps exceeds num_train_timesteps")
        sp = self.config.timestep_spacing
        if sp == "leading":
            ratio = T // num_inference_steps
            ts = (np.arange(0, num_inference_steps) * ratio).round()[::-1].copy().astype(np.int64) + self.config.steps_offset
        elif sp == "linspace":
            ts = np.linspace(0, T - 1, num_inference_steps).round()[::-1].copy().astype(np.int64)
        elif sp == "trailing":
            ts = np.round(np.arange(T, 0, -T / num_inference_steps)).astype(np.int64) - 1
        else:
            raise ValueError(sp)
        self._refuse_epsilon_at_zero_snr(ts)
        self._set(ts, device)

    def coefficients(self, timestep: int):
        """(c_x, c_e, d_x, d_e): prev = c_x*x + c_e*m, x0 = d_x*x + d_e*m for the model output m (A.7 KATs)."""
        t = int(timestep)
        prev_t = t - self.config.num_train_timesteps // self.num_inference_steps
        a = float(self.alphas_cumprod[t])
        ap = float(self.alphas_cumprod[prev_t]) if prev_t >= 0 else self.final_alpha_cumprod
        dx, de, ex, ee = prediction_coefs(self.config.prediction_type, math.sqrt(a), math.sqrt(1.0 - a))
        cx = math.sqrt(ap) * dx + math.sqrt(1.0 - ap) * ex
        ce = math.sqrt(ap) * de + math.sqrt(1.0 - ap) * ee
        return cx, ce, dx, de

    def step_fused(self, model_output, guidance_scale, sample, timestep, cfg=True, eta=0.0, generator=None,
                   guidance_rescale: float = 0.0, inpaint=None, pag_scale=None, sag_scale=None):
        if eta != 0.0:
            raise NotImplementedError("DDIM eta != 0 is never used by the reference (src/models.py:43)")
        if self.num_inference_steps is None:
            raise ValueError("run set_timesteps first")
        cx, ce, dx, de = self.coefficients(timestep)
        e, x = self._prep(model_output), self._prep(sample)
        k = self._rescale(e, cfg, guidance_scale, guidance_rescale, x, pag_scale, sag_scale)
        prev, x0, _ = self._launch(e, cfg, guidance_scale, x, None, None, None, (cx, ce, 0, 0, 0, dx, de, 0, 0), k=k,
                                   **self._blend_kw(inpaint, x), **self._pag_kw(pag_scale, sag_scale, guidance_rescale))
        return prev, x0


def alpha_sigma_lambda(sigma: float):
    """(alpha_t, sigma_t, lambda_t) of a sigma of the table: alpha_t = 1 / sqrt(sigma^2 + 1), sigma_t = sigma alpha_t,
    lambda_t = log alpha_t - log sigma_t (inf at sigma 0)."""
    alpha = 1.0 / math.sqrt(sigma * sigma + 1.0)
    sh = sigma * alpha
    lam = math.log(alpha) - math.log(sh) if sh > 0 else math.inf
    return alpha, sh, lam


def sigma_to_t(sigma, log_sigmas: np.ndarray) -> np.ndarray:
    """upstream's ``_sigma_to_t``: the (fractional) training timestep of a sigma, by piecewise-linear interpolation in
    log-sigma over the training table ``log_sigmas`` (ascending in t)."""
    log_sigma = np.log(np.maximum(np.atleast_1d(np.asarray(sigma, dtype=np.float64)), 1e-10))
    dists = log_sigma[np.newaxis, :] - log_sigmas[:, np.newaxis]
    low_idx = np.cumsum(dists >= 0, axis=0).argmax(axis=0).clip(max=log_sigmas.shape[0] - 2)
    high_idx = low_idx + 1
    low, high = log_sigmas[low_idx], log_sigmas[high_idx]
    w = np.clip((low - log_sigma) / (low - high), 0, 1)
    return (1 - w) * low_idx + w * high_idx


def karras_schedule(train_sigmas: np.ndarray, n: int, rho: float = 7.0):
    """``use_karras_sigmas`` (Karras et al. 2022, eq. 5, rho = 7, as upstream's ``_convert_to_karras``): n sigmas from
    sigma_max = train_sigmas[-1] (t = T - 1) down to sigma_min = train_sigmas[0] (t = 0), and their rounded timesteps
    (``sigma_to_t``; duplicates are legal).  Returns (timesteps int64, sigmas float64)."""
    smax, smin = float(train_sigmas[-1]), float(train_sigmas[0])
    ramp = np.linspace(0, 1, n)
    lo, hi = smin ** (1.0 / rho), smax ** (1.0 / rho)
    sig = (hi + ramp * (lo - hi)) ** rho
    ts = sigma_to_t(sig, np.log(np.asarray(train_sigmas, dtype=np.float64))).round().astype(np.int64)
    return ts, sig


class _SigmaTableScheduler(_FusedStepScheduler):
    """What DPM-Solver and UniPC share: the sigma table over the inference timesteps (the three spacings or Karras sigmas,
    then the final sigma), the zero-terminal-SNR floor, ``add_noise`` from that table, and the multistep bookkeeping
    (``model_outputs`` oldest ... newest, ``lower_order_nums``, the step index)."""
    sigmas: Optional[np.ndarray] = None
    # with rescale_betas_zero_snr and epsilon prediction: the alpha_bar at or below which ``set_timesteps`` refuses a
    # schedule.  0.0 is below the 2^-24 that ``_floor_zero_snr`` writes, so it never refuses there.
    _zero_snr_refusal = 0.0

    def _floor_zero_snr(self):
        if self.config.rescale_betas_zero_snr:
            # as upstream: close to 0 without being 0, so that the first sigma is finite
            self.alphas_cumprod[-1] = 2 ** -24

    def _reset(self):
        self.model_outputs: List[Optional[torch.Tensor]] = [None] * self.config.solver_order
        self.lower_order_nums = 0

    def set_timesteps(self, num_inference_steps: Optional[int] = None, device=None, timesteps=None):
        """``timesteps``: custom schedule, as diffusers 0.32.1 accepts it and the two-scheduler pipeline uses it
        (``src/models.py:488-492``).  ``use_karras_sigmas``: the Karras table of ``karras_schedule`` (upstream-recall)."""
        ts, self.sigmas = self._sigma_table(num_inference_steps, timesteps)
        self._refuse_epsilon_at_zero_snr(ts, floor=self._zero_snr_refusal if self.config.rescale_betas_zero_snr else 0.0)
        self._set(ts, device)
        self._reset()

    def _begin_step(self, timestep) -> int:
        if self.num_inference_steps is None:
            raise ValueError("Number of inference steps is 'None', you need to run 'set_timesteps' after creating the scheduler")
        if self._step_index is None:
            self._step_index = self._index_of(timestep)
        return self._step_index

    def _end_step(self, m):
        """Push the step's history entry (in place: ``models._push_history`` shifts the same list) and advance."""
        self.model_outputs.pop(0)
        self.model_outputs.append(m)
        if self.lower_order_nums < self.config.solver_order:
            self.lower_order_nums += 1
        self._step_index += 1

    def _sigma_table(self, num_inference_steps: Optional[int], timesteps=None):
        """(timesteps int64, sigmas float32 with the final sigma appended) as upstream's ``set_timesteps`` builds them."""
        c = self.config
        T = c.num_train_timesteps
        last = T
        if num_inference_steps is None and timesteps is None:
            raise ValueError("Must pass exactly one of `num_inference_steps` or `timesteps`.")
        karras = bool(c.get("use_karras_sigmas", False))
        if timesteps is not None and karras:
            raise ValueError("Cannot use `timesteps` with `config.use_karras_sigmas = True`")
        ac = self.alphas_cumprod
        sig = np.array(((1 - ac) / ac) ** 0.5)
        if karras:
            ts, sig = karras_schedule(sig, num_inference_steps)      # (timestep_spacing is not read, as upstream)
        else:
            if timesteps is not None:
                ts = np.array([int(t) for t in timesteps]).astype(np.int64)
            elif c.timestep_spacing == "linspace":
                ts = np.linspace(0, last - 1, num_inference_steps + 1).round()[::-1][:-1].copy().astype(np.int64)
            elif c.timestep_spacing == "leading":
                ratio = last // (num_inference_steps + 1)
                ts = (np.arange(0, num_inference_steps + 1) * ratio).round()[::-1][:-1].copy().astype(np.int64) + c.steps_offset
            elif c.timestep_spacing == "trailing":
                ts = np.arange(last, 0, -T / num_inference_steps).round().copy().astype(np.int64) - 1
            else:
                raise ValueError(c.timestep_spacing)
            sig = np.interp(ts, np.arange(0, len(sig)), sig)
        if c.final_sigmas_type == "sigma_min":
            sig_last = ((1 - ac[0]) / ac[0]) ** 0.5
        elif c.final_sigmas_type == "zero":
            sig_last = 0
        else:
            raise ValueError(c.final_sigmas_type)
        return ts, np.concatenate([sig, [sig_last]]).astype(np.float32)

    _alpha_sigma_lambda = staticmethod(alpha_sigma_lambda)

    def _add_noise_coefs(self, timestep):
        """alpha_t, sigma_t of the scheduler's OWN sigma table at the index the loop begins at (upstream's
        DPMSolverMultistepScheduler.add_noise with begin_index set; the table is interpolated, so this is not
        sqrt(alpha_bar) of the fp32 table bit for bit)."""
        alpha, sigma, _ = self._alpha_sigma_lambda(float(self.sigmas[self._index_of(timestep)]))
        return alpha, sigma


@schedulers_registry.add_to_registry("dpm_solver_scheduler")
class DPMSolverScheduler(_SigmaTableScheduler):
    """The reference's ``DPMSolverScheduler`` (``src/schedulers.py:12-187``): multistep
    DPM-Solver / DPM-Solver++ orders 1-3 whose ``step`` also returns the x0 prediction.

    Appendix-B quirk #2 of SURVEY.md: the reference unpacks two values from
    ``convert_model_output`` although its ``++`` branch returns one tensor; the intended behaviour
    implemented here is ``model_output := x0_pred`` for ``++`` and ``(epsilon, x0_pred)`` for
    ``dpmsolver``.  The SDE variants (``sde-dpmsolver`` / ``sde-dpmsolver++``, ``src/schedulers.py:134-147``)
    add a Gaussian term through the kernel's noise coefficient: drawn from ``generator`` per step, or taken
    from ``variance_noise``.  Thresholding is off the hot path.
    """
    _own_defaults = dict(num_train_timesteps=1000, beta_start=0.0001, beta_end=0.02, beta_schedule="linear",
                         trained_betas=None, solver_order=2, prediction_type="epsilon", thresholding=False,
                         algorithm_type="dpmsolver++", solver_type="midpoint", lower_order_final=True,
                         euler_at_final=False, final_sigmas_type="zero", timestep_spacing="linspace", steps_offset=0,
                         rescale_betas_zero_snr=False, use_karras_sigmas=False)
    _accepted = tuple(_own_defaults)

    def __init__(self, **kwargs):
        super().__init__(**kwargs)
        c = self.config
        if c.algorithm_type not in ("dpmsolver", "dpmsolver++", "sde-dpmsolver", "sde-dpmsolver++"):
            raise NotImplementedError(f"{c.algorithm_type} is not implemented for {self.__class__}")
        if c.algorithm_type not in ("dpmsolver++", "sde-dpmsolver++") and c.final_sigmas_type == "zero":
            raise ValueError(f"`final_sigmas_type` {c.final_sigmas_type} is not supported for `algorithm_type` "
                             f"{c.algorithm_type}. Please choose `sigma_min` instead.")
        if c.solver_type != "midpoint" or c.thresholding:
            raise NotImplementedError("only midpoint / no thresholding is on the hot path")
        self._check_prediction_type()
        self._floor_zero_snr()
        if c.solver_order not in (1, 2, 3):
            raise ValueError("solver_order must be 1, 2 or 3")
        self._reset()

    def _convert_coefs(self, i: int):
        a0, s0, _ = self._alpha_sigma_lambda(float(self.sigmas[i]))
        dx, de, ex, ee = prediction_coefs(self.config.prediction_type, a0, s0)
        if self.config.algorithm_type in ("dpmsolver++", "sde-dpmsolver++"):        # src/schedulers.py:35
            return dx, de, dx, de                         # history entry m := x0
        # history entry m := eps (:64); x0 = (x - sigma_t eps) / alpha_t from that eps (:94)
        return (1.0 - s0 * ex) / a0, -s0 * ee / a0, ex, ee

    def convert_model_output(self, model_output, *args, sample=None, **kwargs):
        """``src/schedulers.py:14-96``: returns (converted_output, x0_pred) at the current step."""
        if sample is None:
            if len(args) > 1:
                sample = args[1]
            else:
                raise ValueError("missing `sample` as a required keyward argument")
        i = self._step_index if self._step_index is not None else 0
        yx, ye, mx, me = self._convert_coefs(i)
        x, e = self._prep(sample), self._prep(model_output)
        _, x0, m = self._launch(e, False, 0.0, x, None, None, None, (1, 0, 0, 0, 0, yx, ye, mx, me),
                                want_y2=True, want_m=True)
        return m, x0

    def _update_coefs(self, i: int, order: int, mx: float, me: float):
        """prev = px*x + pe*eps + p1*m1 + p2*m2 + pn*z for the order-`order` multistep update (A.6.2); the SDE
        variants (z ~ N(0, I)) use the same linear form with their own kA/kB/kC and a noise coefficient."""
        alg = self.config.algorithm_type
        pp = alg in ("dpmsolver++", "sde-dpmsolver++")
        sde = alg.startswith("sde-")
        a_t, s_t, l_t = self._alpha_sigma_lambda(float(self.sigmas[i + 1]))
        a_0, s_0, l_0 = self._alpha_sigma_lambda(float(self.sigmas[i]))
        h = l_t - l_0
        pn = 0.0
        if pp and not sde:
            ratio = s_t / s_0
            em1 = math.expm1(-h) if math.isfinite(h) else -1.0       # e^{-h} - 1
            kA = -a_t * em1
        elif not sde:
            ratio = a_t / a_0
            em1 = math.expm1(h)
            kA = -s_t * em1
        elif pp:                                                     # sde-dpmsolver++
            e2 = math.expm1(-2.0 * h) if math.isfinite(h) else -1.0   # e^{-2h} - 1
            ratio = s_t / s_0 * (math.exp(-h) if math.isfinite(h) else 0.0)
            kA = -a_t * e2
            pn = s_t * math.sqrt(-e2)
        else:                                                        # sde-dpmsolver
            ratio = a_t / a_0
            kA = -2.0 * s_t * math.expm1(h)
            pn = s_t * math.sqrt(math.expm1(2.0 * h))
        c0, c1, c2 = kA, 0.0, 0.0
        if order >= 2:
            _, _, l_1 = self._alpha_sigma_lambda(float(self.sigmas[i - 1]))
            r0 = (l_0 - l_1) / h
        if order == 2:
            c0 = kA * (1.0 + 0.5 / r0)
            c1 = -0.5 * kA / r0
        elif order == 3:
            _, _, l_2 = self._alpha_sigma_lambda(float(self.sigmas[i - 2]))
            r1 = (l_1 - l_2) / h
            if sde and not pp:
                raise NotImplementedError("sde-dpmsolver has no third-order update (as upstream)")
            if sde:
                kB = a_t * (e2 / (2.0 * h) + 1.0)
                kC = a_t * ((-e2 - 2.0 * h) / (4.0 * h * h) - 0.5)
            elif pp:
                kB = a_t * (em1 / h + 1.0)
                kC = -a_t * ((em1 + h) / (h * h) - 0.5)
            else:
                kB = -s_t * (em1 / h - 1.0)
                kC = -s_t * ((em1 - h) / (h * h) - 0.5)
            rho = r0 / (r0 + r1)
            u = kB * (1.0 + rho) + kC / (r0 + r1)
            v = -kB * rho - kC / (r0 + r1)
            c0 = kA + u / r0
            c1 = -u / r0 + v / r1
            c2 = -v / r1
        return ratio + c0 * mx, c0 * me, c1, c2, pn

    def step_fused(self, model_output, guidance_scale, sample, timestep, cfg=True, eta=0.0, generator=None,
                   variance_noise: Optional[torch.Tensor] = None, guidance_rescale: float = 0.0, inpaint=None, pag_scale=None, sag_scale=None):
        c = self.config
        i, n = self._begin_step(timestep), len(self._timesteps_list)
        lower_order_final = (i == n - 1) and (c.euler_at_final or (c.lower_order_final and n < 15)
                                              or c.final_sigmas_type == "zero")
        lower_order_second = (i == n - 2) and c.lower_order_final and n < 15
        if c.solver_order == 1 or self.lower_order_nums < 1 or lower_order_final:
            order = 1
        elif c.solver_order == 2 or self.lower_order_nums < 2 or lower_order_second:
            order = 2
        else:
            order = 3
        yx, ye, mx, me = self._convert_coefs(i)
        px, pe, p1, p2, pn = self._update_coefs(i, order, mx, me)
        hist = self.model_outputs                      # oldest ... newest
        m1 = hist[-1] if order >= 2 else None
        m2 = hist[-2] if order >= 3 else None
        x = self._prep(sample)
        z = None
        if c.algorithm_type.startswith("sde-"):        # src/schedulers.py:134-147
            if variance_noise is None:
                variance_noise = sdist.randn(x.shape, generator)
            z = self._prep(variance_noise.to(x.device))
        e = self._prep(model_output)
        k = self._rescale(e, cfg, guidance_scale, guidance_rescale, x, pag_scale, sag_scale)
        # (inpainting: the history entry m0 and x0 are taken before the blend, as upstream steps first and blends after)
        prev, x0, m0 = self._launch(e, cfg, guidance_scale, x, m1, m2, z, (px, pe, p1, p2, pn, yx, ye, mx, me),
                                    want_y2=True, want_m=True, k=k, **self._blend_kw(inpaint, x), **self._pag_kw(pag_scale, sag_scale, guidance_rescale))
        self._end_step(m0)
        return prev, x0


@schedulers_registry.add_to_registry("lcm_scheduler")
class LCMScheduler(_FusedStepScheduler):
    """diffusers ``LCMScheduler`` (A.6.3): consistency step with boundary-condition scalings and
    re-noising by a fresh Gaussian on every step but the last."""
    _own_defaults = dict(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear",
                         trained_betas=None, original_inference_steps=50, clip_sample=False, set_alpha_to_one=True,
                         steps_offset=0, prediction_type="epsilon", thresholding=False, timestep_spacing="leading",
                         timestep_scaling=10.0, rescale_betas_zero_snr=False)
    _accepted = tuple(_own_defaults)

    def __init__(self, **kwargs):
        super().__init__(**kwargs)
        if self.config.clip_sample or self.config.thresholding:
            raise NotImplementedError("clip_sample / thresholding are not on the hot path")
        self._check_prediction_type()

    def set_timesteps(self, num_inference_steps: int, device=None, original_inference_steps=None):
        c = self.config
        original = original_inference_steps or c.original_inference_steps
        if num_inference_steps > original:
            raise ValueError("num_inference_steps cannot exceed original_inference_steps")
        k = c.num_train_timesteps // original
        origin = (np.asarray(list(range(1, int(original) + 1))) * k - 1)[::-1].copy()
        idx = np.floor(np.linspace(0, len(origin), num=num_inference_steps, endpoint=False)).astype(np.int64)
        self._refuse_epsilon_at_zero_snr(origin[idx])
        self._set(origin[idx], device)

    def step_fused(self, model_output, guidance_scale, sample, timestep, cfg=True, eta=0.0, generator=None,
                   noise: Optional[torch.Tensor] = None, guidance_rescale: float = 0.0, inpaint=None, pag_scale=None, sag_scale=None):
        if self.num_inference_steps is None:
            raise ValueError("run set_timesteps first")
        if self._step_index is None:
            self._step_index = self._index_of(timestep)
        i = self._step_index
        t = int(timestep)
        prev_t = self._timesteps_list[i + 1] if i + 1 < len(self._timesteps_list) else t
        a = float(self.alphas_cumprod[t])
        ap = float(self.alphas_cumprod[prev_t]) if prev_t >= 0 else self.final_alpha_cumprod
        st = t * self.config.timestep_scaling
        c_skip = 0.25 / (st * st + 0.25)
        c_out = st / math.sqrt(st * st + 0.25)
        dx, de, _, _ = prediction_coefs(self.config.prediction_type, math.sqrt(a), math.sqrt(1.0 - a))
        yx, ye = c_out * dx + c_skip, c_out * de            # "denoised"
        x = self._prep(sample)
        last = i == self.num_inference_steps - 1
        if last:
            coef, z = (yx, ye, 0, 0, 0, yx, ye, 0, 0), None
        else:
            if noise is None:
                noise = sdist.randn(x.shape, generator)
            z = self._prep(noise.to(x.device))
            coef = (math.sqrt(ap) * yx, math.sqrt(ap) * ye, 0, 0, math.sqrt(1.0 - ap), yx, ye, 0, 0)
        e = self._prep(model_output)
        k = self._rescale(e, cfg, guidance_scale, guidance_rescale, x, pag_scale, sag_scale)
        prev, den, _ = self._launch(e, cfg, guidance_scale, x, None, None, z, coef, k=k, **self._blend_kw(inpaint, x),
                                    **self._pag_kw(pag_scale, sag_scale, guidance_rescale))
        self._step_index += 1
        return prev, den


@schedulers_registry.add_to_registry("pndm_scheduler")
class PNDMScheduler(_FusedStepScheduler):
    """diffusers ``PNDMScheduler`` with ``skip_prk_steps=True`` (PLMS) -- the scheduler the SD-1.5
    checkpoint ships and that the reference's ``deep_cache`` / ``default`` methods therefore run
    (``src/experiments/deep_cache.py:17-18``, ``default_sd.py:15-16``).
    N inference steps = N+1 UNet calls (second timestep duplicated).  Every PLMS update is a linear
    combination of the sample, the current and up to three earlier noise predictions, so it runs on
    the same fused kernel; ``step`` returns a 1-tuple like upstream."""
    _own_defaults = dict(num_train_timesteps=1000, beta_start=0.0001, beta_end=0.02, beta_schedule="linear",
                         trained_betas=None, skip_prk_steps=False, set_alpha_to_one=False, prediction_type="epsilon",
                         timestep_spacing="leading", steps_offset=0)
    _accepted = tuple(_own_defaults)

    def __init__(self, **kwargs):
        super().__init__(**kwargs)
        if not self.config.skip_prk_steps or self.config.timestep_spacing != "leading":
            raise NotImplementedError("only the SD-1.5 PLMS configuration (skip_prk_steps, leading) is built")
        if self.config.prediction_type not in ("epsilon", "v_prediction"):       # as upstream's _get_prev_sample
            raise ValueError(f"prediction_type given as {self.config.prediction_type} must be one of `epsilon` or "
                             "`v_prediction`")
        self.ets: List[torch.Tensor] = []
        self.counter = 0
        self.cur_sample = None

    def set_timesteps(self, num_inference_steps: int, device=None):
        T = self.config.num_train_timesteps
        ratio = T // num_inference_steps
        base = (np.arange(0, num_inference_steps) * ratio).round() + self.config.steps_offset
        plms = np.concatenate([base[:-1], base[-2:-1], base[-1:]])[::-1].copy().astype(np.int64)
        self._set(plms, device)
        self.num_inference_steps = num_inference_steps        # N, not len(timesteps) = N + 1
        self.ets, self.counter, self.cur_sample = [], 0, None

    def _prev_coefs(self, t: int, prev_t: int):
        """(sample coefficient, model-output coefficient) of ``_get_prev_sample``.  v-prediction: upstream converts the
        PLMS-combined output m to eps = sqrt(a_t)*m + sqrt(1 - a_t)*sample there, which is folded into the two."""
        a_t = float(self.alphas_cumprod[t])
        a_p = float(self.alphas_cumprod[prev_t]) if prev_t >= 0 else self.final_alpha_cumprod
        sample_coeff = math.sqrt(a_p / a_t)
        denom = a_t * math.sqrt(1 - a_p) + math.sqrt(a_t * (1 - a_t) * a_p)
        k = -(a_p - a_t) / denom
        if self.config.prediction_type == "v_prediction":
            return sample_coeff + k * math.sqrt(1.0 - a_t), k * math.sqrt(a_t)
        return sample_coeff, k

    def step_fused(self, model_output, guidance_scale, sample, timestep, cfg=True, eta=0.0, generator=None,
                   guidance_rescale: float = 0.0, inpaint=None, pag_scale=None, sag_scale=None):
        if inpaint is not None:
            raise NotImplementedError("PNDMScheduler: the latent blend of inpainting is not built (its second timestep is "
                                      "duplicated; DDIM, DPM-Solver and LCM are built)")
        if self.num_inference_steps is None:
            raise ValueError("run set_timesteps first")
        t = int(timestep)
        ratio = self.config.num_train_timesteps // self.num_inference_steps
        prev_t = t - ratio
        x = self._prep(sample)
        e = self._prep(model_output)
        kr = self._rescale(e, cfg, guidance_scale, guidance_rescale, x, pag_scale, sag_scale)
        hist = self.ets
        if self.counter != 1:
            n_hist = min(len(hist), 3)
            w = {0: (1.0,), 1: (1.5, -0.5), 2: (23 / 12, -16 / 12, 5 / 12), 3: (55 / 24, -59 / 24, 37 / 24, -9 / 24)}[n_hist]
            sc, k = self._prev_coefs(t, prev_t)
            ms = [hist[-1 - i] if i < n_hist else None for i in range(3)]
            ws = [w[i + 1] if i < n_hist else 0.0 for i in range(3)]
            prev, _, e_out = self._launch(e, cfg, guidance_scale, x, ms[0], ms[1], None,
                                          (sc, k * w[0], k * ws[0], k * ws[1], 0, 0, 0, 0.0, 1.0, k * ws[2]),
                                          want_y2=False, want_m=True, m3=ms[2], k=kr, **self._pag_kw(pag_scale, sag_scale, guidance_rescale))
            self.ets = (hist + [e_out])[-4:]
            if self.counter == 0:
                self.cur_sample = x
        else:
            # second call (same timestep again): average with the first prediction, restart from cur_sample
            sc, k = self._prev_coefs(t + ratio, t)
            prev, _, _ = self._launch(e, cfg, guidance_scale, self.cur_sample, hist[-1], None, None,
                                      (sc, 0.5 * k, 0.5 * k, 0, 0, 0, 0, 0, 0, 0), want_y2=False, want_m=False, k=kr, **self._pag_kw(pag_scale, sag_scale, guidance_rescale))
            self.cur_sample = None
        self.counter += 1
        return (prev,)

    def add_noise(self, original_samples, noise, timestep):
        raise NotImplementedError("PNDMScheduler: starting part-way down the schedule (image-to-image) is not built -- its "
                                  "second timestep is duplicated, and slicing the list changes what the PLMS warm-up means")

    def step(self, model_output, timestep, sample, return_dict: bool = False, **kwargs):
        out_dtype = model_output.dtype
        (prev,) = self.step_fused(model_output, 0.0, sample, timestep, cfg=False)
        return (prev.to(out_dtype),)


UNIPC_SOLVER_TYPES = ("bh1", "bh2")


def _unipc_update(lam_s0: float, lam_t: float, lam_hist, order: int, solver_type: str, predict_x0: bool, corrector: bool,
                  a_t: float, s_t: float, a_s0: float, s_s0: float):
    """One UniPC update from (lambda_s0) to (lambda_t) as coefficients: returns (A, c_m0, [c_m1, c_m2], c_new) with
        out = A*x + c_m0*m0 + sum_k c_mk*m_k + c_new*m_new
    m0 the model output at s0, m_k the ones before it (``lam_hist``: their lambdas, ``order - 1`` of them), m_new the model
    output at t (corrector only; 0 for the predictor).  upstream's recurrences (rks, R, b, B_h, h_phi_k), with the D1
    differences (m_k - m0) / r_k folded into the coefficients.  fp64, no torch."""
    h = lam_t - lam_s0
    if not math.isfinite(h):
        # the step onto sigma 0 (lambda_t = inf), in the limit: sigma_t -> 0, e^{-h} -> 0, sigma_t e^{h} -> alpha_t sigma_s0 /
        # alpha_s0.  First order only: the higher-order terms diverge there (upstream returns NaN).
        if corrector or order != 1:
            raise ValueError("UniPC: a step onto sigma 0 is first-order (lower_order_final=False with final_sigmas_type="
                             "'zero' and solver_order > 1 has no finite update; use final_sigmas_type='sigma_min')")
        if predict_x0:
            return 0.0, a_t, [], 0.0
        return a_t / a_s0, -(a_t * s_s0 / a_s0), [], 0.0
    hh = -h if predict_x0 else h
    h_phi_1 = math.expm1(hh)
    if solver_type == "bh1":
        B_h = hh
    elif solver_type == "bh2":
        B_h = h_phi_1
    else:
        raise NotImplementedError(f"solver_type {solver_type!r}: {UNIPC_SOLVER_TYPES} are built")
    rks = [(l - lam_s0) / h for l in lam_hist] + [1.0]
    R, b = [], []
    h_phi_k = h_phi_1 / hh - 1.0
    factorial_i = 1
    for i in range(1, order + 1):
        R.append([rk ** (i - 1) for rk in rks])
        b.append(h_phi_k * factorial_i / B_h)
        factorial_i *= i + 1
        h_phi_k = h_phi_k / hh - 1.0 / factorial_i
    if corrector:
        rhos = [0.5] if order == 1 else list(np.linalg.solve(np.array(R, dtype=np.float64), np.array(b, dtype=np.float64)))
        rho_hist, rho_new = rhos[:-1], rhos[-1]
    else:
        if order == 1:
            rho_hist = []
        elif order == 2:
            rho_hist = [0.5]
        else:
            rho_hist = list(np.linalg.solve(np.array(R, dtype=np.float64)[:-1, :-1], np.array(b, dtype=np.float64)[:-1]))
        rho_new = 0.0
    A, S = (s_t / s_s0, a_t) if predict_x0 else (a_t / a_s0, s_t)
    c_hist = [-S * B_h * rho / rk for rho, rk in zip(rho_hist, rks[:-1])]
    c_new = -S * B_h * rho_new
    c_m0 = -S * h_phi_1 - sum(c_hist) - c_new
    return A, c_m0, [float(v) for v in c_hist], float(c_new)


def unipc_rows(sigmas, i: int, corrector_order: int, predictor_order: int, solver_type: str = "bh2", predict_x0: bool = True,
               prediction_type: str = "epsilon"):
    """The coefficient rows (cm, cy, cc, cp) of ``sd_sched_step_pc`` for step ``i`` of the sigma table ``sigmas`` (n + 1
    entries): the conversion at sigma_i, the corrector of order ``corrector_order`` from sigma_(i-1) to sigma_i (0: no
    corrector, cc is None) and the predictor of order ``predictor_order`` from sigma_i to sigma_(i+1).  Pure host
    arithmetic in fp64."""
    asl = {j: alpha_sigma_lambda(float(sigmas[j])) for j in range(max(i - 3, 0), i + 2)}      # (the entries a step can read)
    a0, s0, l0 = asl[i]
    dx, de, ex, ee = prediction_coefs(prediction_type, a0, s0)
    cy = (dx, de)
    cm = (dx, de) if predict_x0 else (ex, ee)
    cc = None
    if corrector_order:
        o = corrector_order
        if not 1 <= o <= 3 or i - o < 0:
            raise ValueError(f"UniPC corrector of order {o} at step {i}")
        ap, sp, lp = asl[i - 1]
        A, c0, ch, cn = _unipc_update(lp, l0, [asl[i - 1 - k][2] for k in range(1, o)], o, solver_type, predict_x0, True,
                                      a0, s0, ap, sp)
        ch = ch + [0.0] * (2 - len(ch))
        cc = (A, c0, ch[0], ch[1], cn)                # x_last, h1, h2, h3, m_t
    o = predictor_order
    if not 1 <= o <= 3 or i - (o - 1) < 0:
        raise ValueError(f"UniPC predictor of order {o} at step {i}")
    at, st, lt = asl[i + 1]
    A, c0, ch, _ = _unipc_update(l0, lt, [asl[i - k][2] for k in range(1, o)], o, solver_type, predict_x0, False,
                                 at, st, a0, s0)
    ch = ch + [0.0] * (2 - len(ch))
    cp = (A, c0, ch[0], ch[1])                        # xc, m_t, h1, h2
    return cm, cy, cc, cp


@schedulers_registry.add_to_registry("unipc_scheduler")
class UniPCScheduler(_SigmaTableScheduler):
    """diffusers' ``UniPCMultistepScheduler`` (Zhao et al. 2023), upstream-recall: restated from the paper and from memory of
    upstream's code, not checked against an installed diffusers.  A step corrects the sample the previous step predicted
    (with this step's model output, so for no extra UNet evaluation) and predicts the next one from the corrected sample;
    both are linear in the sample, the model output and the history, so the step is ONE ``sd_sched_step_pc`` launch whose
    coefficient rows ``unipc_rows`` derives in fp64.  The sigma table, spacings, final sigma and zero-SNR handling are
    ``DPMSolverScheduler``'s.  Not built: thresholding, ``solver_p``, the beta / exponential / flow sigma options."""
    _own_defaults = dict(num_train_timesteps=1000, beta_start=0.0001, beta_end=0.02, beta_schedule="linear",
                         trained_betas=None, solver_order=2, prediction_type="epsilon", thresholding=False,
                         predict_x0=True, solver_type="bh2", lower_order_final=True, disable_corrector=[],
                         timestep_spacing="linspace", steps_offset=0, final_sigmas_type="zero",
                         rescale_betas_zero_snr=False, use_karras_sigmas=False)
    _accepted = tuple(_own_defaults)
    # (the 2^-24 that stands for alpha_bar = 0 is refused like the 0: x0 = (x - sigma eps) / 2^-12 there)
    _zero_snr_refusal = 2 ** -24

    def __init__(self, **kwargs):
        super().__init__(**kwargs)
        c = self.config
        if c.thresholding:
            raise NotImplementedError("thresholding is not on the hot path")
        if c.solver_type not in UNIPC_SOLVER_TYPES:
            raise NotImplementedError(f"solver_type {c.solver_type!r}: {UNIPC_SOLVER_TYPES} are built")
        if c.solver_order not in (1, 2, 3):
            raise ValueError(f"solver_order={c.solver_order!r} must be 1, 2 or 3")
        if c.final_sigmas_type not in ("zero", "sigma_min"):
            raise ValueError(f"final_sigmas_type {c.final_sigmas_type!r}: 'zero' or 'sigma_min'")
        self._check_prediction_type()
        self._floor_zero_snr()
        self.config["disable_corrector"] = [int(v) for v in (c.disable_corrector or [])]
        self._reset()

    def _reset(self):
        super()._reset()
        self.last_sample: Optional[torch.Tensor] = None
        self.this_order = 0

    def step_orders(self, i: int):
        """(corrector order or 0, predictor order) of step ``i`` given the state, in upstream's order: the corrector runs
        unless this is the first executed step of the call or step i - 1 is in ``disable_corrector``, at the previous step's
        order; the predictor's order is min(solver_order, steps left) under ``lower_order_final``, capped by the history."""
        c = self.config
        use_corrector = self.last_sample is not None and i > 0 and (i - 1) not in c.disable_corrector
        this_order = min(c.solver_order, len(self._timesteps_list) - i) if c.lower_order_final else c.solver_order
        return (self.this_order if use_corrector else 0), min(this_order, self.lower_order_nums + 1)

    def rows(self, i: int, corrector_order: int, predictor_order: int):
        c = self.config
        return unipc_rows(self.sigmas, i, corrector_order, predictor_order, c.solver_type, c.predict_x0, c.prediction_type)

    @staticmethod
    def _launch_pc(eps, cfg, guidance, x, x_last, hist, rows, k=None, blend=None, pag=None, sag=None):
        """ONE ``sd_sched_step_pc`` launch (``pag``, the step's PAG scale: ``sd_sched_step_pc_pag``, eps = [u | c | p] or [c | p]).  ``hist``: (h1, h2, h3), newest first, None where the row has no weight;
        ``rows`` = (cm, cy, cc, cp) of ``unipc_rows``.  Returns (prev, x_corr, y2, m_t)."""
        lib = _lib.load()
        cm, cy, cc, cp = rows
        n = x.numel()
        prev, xc, y2, mo = (torch.empty_like(x) for _ in range(4))
        carr = (C.c_float * 13)(*[float(v) for v in (*cm, *cy, *(cc if cc is not None else (0.0,) * 5), *cp)])
        init = bnoise = mask = None
        a, s, hw = 1.0, 0.0, 0
        if blend is not None:
            init, bnoise, mask, a, s = blend
            hw = mask.numel() // mask.shape[0]
        tail = (x.data_ptr(), _lib.ptr(x_last), _lib.ptr(hist[0]), _lib.ptr(hist[1]), _lib.ptr(hist[2]), prev.data_ptr(), xc.data_ptr(),
                y2.data_ptr(), mo.data_ptr(), carr, n, _lib.ptr(k), n // x.shape[0], _lib.ptr(init), _lib.ptr(bnoise), _lib.ptr(mask),
                float(a), float(s), int(hw))
        if sag is not None:
            _lib.check(lib.sd_sched_step_pc_sag(_lib.current_stream(), eps.data_ptr(), GUIDE_CFG_SAG if cfg else GUIDE_SAG,
                                                float(guidance), float(sag), *tail), "sd_sched_step_pc_sag")
        elif pag is not None:
            _lib.check(lib.sd_sched_step_pc_pag(_lib.current_stream(), eps.data_ptr(), GUIDE_CFG_PAG if cfg else GUIDE_PAG,
                                                float(guidance), float(pag), *tail), "sd_sched_step_pc_pag")
        else:
            _lib.check(lib.sd_sched_step_pc(_lib.current_stream(), eps.data_ptr(), int(cfg), float(guidance), *tail),
                       "sd_sched_step_pc")
        return prev, xc, y2, mo

    def step_fused(self, model_output, guidance_scale, sample, timestep, cfg=True, eta=0.0, generator=None,
                   guidance_rescale: float = 0.0, inpaint=None, pag_scale=None, sag_scale=None):
        """``eta`` and ``generator`` are not read (the solver is deterministic)."""
        i = self._begin_step(timestep)
        order_c, order_p = self.step_orders(i)
        rows = self.rows(i, order_c, order_p)
        newest_first = self.model_outputs[::-1]
        depth = max(order_c, order_p - 1)                       # the corrector reads h1..h_o, the predictor h1..h_(o-1)
        hist = [newest_first[j] if j < min(depth, len(newest_first)) else None for j in range(3)]
        e, x = self._prep(model_output), self._prep(sample)
        k = self._rescale(e, cfg, guidance_scale, guidance_rescale, x, pag_scale, sag_scale)
        # (inpainting: the corrected sample, the history entry and x0 are taken before the blend, as upstream steps first)
        prev, xc, x0, m_t = self._launch_pc(e, cfg, guidance_scale, x, self.last_sample if order_c else None, hist, rows,
                                            k=k, blend=self._blend(inpaint, x), **self._pag_kw(pag_scale, sag_scale, guidance_rescale))
        self.last_sample = xc
        self.this_order = order_p
        self._end_step(m_t)
        return prev, x0


# the checkpoint's scheduler class (``_class_name`` of scheduler/scheduler_config.json) -> its registry key
CHECKPOINT_SCHEDULERS = {"PNDMScheduler": "pndm_scheduler", "DDIMScheduler": "ddim_scheduler",
                         "DPMSolverMultistepScheduler": "dpm_solver_scheduler", "LCMScheduler": "lcm_scheduler",
                         "UniPCMultistepScheduler": "unipc_scheduler"}


def checkpoint_scheduler_name(config) -> str:
    """Registry key of the scheduler class a checkpoint's config names (PNDM when it names none, as SD-1.5 ships);
    raises NotImplementedError for a class that is not built."""
    cls = config.get("_class_name", "PNDMScheduler")
    if cls not in CHECKPOINT_SCHEDULERS:
        raise NotImplementedError(f"the checkpoint's scheduler class {cls!r} is not built "
                                  f"(built: {sorted(CHECKPOINT_SCHEDULERS)})")
    return CHECKPOINT_SCHEDULERS[cls]


class PNDMConfigStub:
    """The checkpoint's scheduler config holder: ``from_config(model.scheduler.config)``
    (``src/experiments/base_experiment.py:69-72``) reads the checkpoint's scheduler config from it -- SD-1.5's PNDM
    config unless a local checkpoint ships its own (``weights.load_scheduler_config``).  Call
    ``schedulers_registry[checkpoint_scheduler_name(stub.config)].from_config(stub.config)`` to actually step with it."""
    order = 1
    init_noise_sigma = 1.0

    def __init__(self, config=None):
        self.config = SchedulerConfig(SD15_SCHEDULER_CONFIG if config is None else config)

    def set_timesteps(self, *a, **k):
        raise NotImplementedError("this is only the checkpoint's scheduler CONFIG; build a scheduler with "
                                  "schedulers_registry[...].from_config(model.scheduler.config)")
