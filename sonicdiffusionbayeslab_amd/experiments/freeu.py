"""``methods_registry["freeu"]``: FreeU (diffusers ``enable_freeu``) swept over factor settings.

The reference's registry has no such method; it is built like ``tome``: one setting per entry of
``experiment_params.freeu`` (a list of dicts ``{s1, s2, b1, b2}``; ``null`` = FreeU off, the plain pipeline), enabled across
the whole sweep of ``num_inference_steps``.  The scheduler is ``scheduler.scheduler_name`` where given, else the
checkpoint's own."""
from ..registry import methods_registry, schedulers_registry
from ..schedulers import checkpoint_scheduler_name
from .base_experiment import BaseMethod


@methods_registry.add_to_registry("freeu")
class FreeUMethod(BaseMethod):
    def setup_exp_params(self):
        ep = self.config.experiment_params
        settings = ep.freeu
        if settings is None or isinstance(settings, (str, bytes)) or hasattr(settings, "keys") or not hasattr(settings, "__iter__"):
            raise ValueError("experiment_params.freeu must be a list of {s1, s2, b1, b2} dicts (null = off)")
        weight_dtype = self.config.model.get("weight_dtype", None) or "bf16"
        self.freeu = [self.parse_freeu({"freeu": s}, weight_dtype) for s in settings]      # refused by name before any GPU work
        self.num_inference_steps = ep.num_inference_steps

    def setup_scheduler(self):
        config = self.model.scheduler.config
        name = self.config.get("scheduler", {}).get("scheduler_name", None) or checkpoint_scheduler_name(config)
        self.model.scheduler = schedulers_registry[name].from_config(config)

    def run_experiment(self):
        for f in self.freeu:
            label = "off" if f is None else "s1={s1} s2={s2} b1={b1} b2={b2}".format(**f)
            if f is None:
                self.model.disable_freeu()
            else:
                self.model.enable_freeu(**f)
            try:
                self.sweep(self.num_inference_steps, lambda n: {"num_inference_steps": n},
                           lambda n: f"Inference steps: {n}, FreeU: {label}",
                           extra=lambda n: {"FreeU": label})
            finally:
                self.model.disable_freeu()
