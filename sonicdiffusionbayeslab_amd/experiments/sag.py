"""``methods_registry["sag"]``: self-attention guidance (SAG) swept over guidance scales.

The reference's registry has no such method; it is built like ``pag``: one setting per entry of
``experiment_params.sag_scale`` (a list of SAG scales; ``null`` = SAG off, the plain pipeline), enabled across the whole
sweep of ``num_inference_steps``.  Optional ``experiment_params.height`` / ``width`` (pixels; absent = the checkpoint's own
size).  The scheduler is ``scheduler.scheduler_name`` where given, else the checkpoint's own."""
from ..models import StableDiffusionModel
from ..registry import methods_registry, schedulers_registry
from ..schedulers import checkpoint_scheduler_name
from .base_experiment import BaseMethod


@methods_registry.add_to_registry("sag")
class SAGMethod(BaseMethod):
    def setup_exp_params(self):
        ep = self.config.experiment_params
        scales = ep.sag_scale
        if scales is None or isinstance(scales, (str, bytes)) or hasattr(scales, "keys") or not hasattr(scales, "__iter__"):
            raise ValueError("experiment_params.sag_scale must be a list of SAG scales (null = off)")
        self.sag_scale = list(scales)
        weight_dtype = self.config.model.get("weight_dtype", None) or "bf16"
        for s in self.sag_scale:            # refused by name before any GPU work
            if s is not None:
                StableDiffusionModel.check_sag_args(s, None, weight_dtype)
        self.size_kwargs = {k: int(ep[k]) for k in ("height", "width") if ep.get(k, None) is not None}
        self.num_inference_steps = ep.num_inference_steps

    def setup_scheduler(self):
        config = self.model.scheduler.config
        name = self.config.get("scheduler", {}).get("scheduler_name", None) or checkpoint_scheduler_name(config)
        self.model.scheduler = schedulers_registry[name].from_config(config)

    def run_experiment(self):
        for s in self.sag_scale:
            label = "off" if s is None else f"scale {s}"
            if s is None:
                self.model.disable_sag()
            else:
                self.model.enable_sag(sag_scale=s)
            try:
                self.sweep(self.num_inference_steps, lambda n: {"num_inference_steps": n, **self.size_kwargs},
                           lambda n: f"Inference steps: {n}, SAG: {label}",
                           extra=lambda n: {"SAG": label})
            finally:
                self.model.disable_sag()
