"""``methods_registry["pag"]``: perturbed-attention guidance (PAG) swept over guidance scales.

The reference's registry has no such method; it is built like ``hypertile``: one setting per entry of
``experiment_params.pag_scale`` (a list of PAG scales; ``null`` = PAG off, the plain pipeline), enabled across the whole
sweep of ``num_inference_steps``.  Optional ``experiment_params.pag_adaptive_scale`` (default 0.0),
``experiment_params.pag_applied_layers`` (a name or a list, default ``"mid"``) and ``experiment_params.height`` / ``width``
(pixels; absent = the checkpoint's own size).  The scheduler is ``scheduler.scheduler_name`` where given, else the
checkpoint's own."""
from ..models import StableDiffusionModel
from ..registry import methods_registry, schedulers_registry
from ..schedulers import checkpoint_scheduler_name
from .base_experiment import BaseMethod


@methods_registry.add_to_registry("pag")
class PAGMethod(BaseMethod):
    def setup_exp_params(self):
        ep = self.config.experiment_params
        scales = ep.pag_scale
        if scales is None or isinstance(scales, (str, bytes)) or hasattr(scales, "keys") or not hasattr(scales, "__iter__"):
            raise ValueError("experiment_params.pag_scale must be a list of PAG scales (null = off)")
        self.pag_scale = list(scales)
        self.pag_adaptive_scale = ep.get("pag_adaptive_scale", 0.0)
        layers = ep.get("pag_applied_layers", "mid")
        self.pag_applied_layers = layers if isinstance(layers, str) else list(layers)
        weight_dtype = self.config.model.get("weight_dtype", None) or "bf16"
        for s in self.pag_scale:            # refused by name before any GPU work
            if s is not None:
                StableDiffusionModel.check_pag_args(s, self.pag_adaptive_scale, self.pag_applied_layers, None, weight_dtype)
        self.size_kwargs = {k: int(ep[k]) for k in ("height", "width") if ep.get(k, None) is not None}
        self.num_inference_steps = ep.num_inference_steps

    def setup_scheduler(self):
        config = self.model.scheduler.config
        name = self.config.get("scheduler", {}).get("scheduler_name", None) or checkpoint_scheduler_name(config)
        self.model.scheduler = schedulers_registry[name].from_config(config)

    def run_experiment(self):
        for s in self.pag_scale:
            label = "off" if s is None else f"scale {s}, adaptive {self.pag_adaptive_scale}, layers {self.pag_applied_layers}"
            if s is None:
                self.model.disable_pag()
            else:
                self.model.enable_pag(pag_scale=s, pag_adaptive_scale=self.pag_adaptive_scale,
                                      pag_applied_layers=self.pag_applied_layers)
            try:
                self.sweep(self.num_inference_steps, lambda n: {"num_inference_steps": n, **self.size_kwargs},
                           lambda n: f"Inference steps: {n}, PAG: {label}",
                           extra=lambda n: {"PAG": label})
            finally:
                self.model.disable_pag()
