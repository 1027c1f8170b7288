"""``methods_registry["tgate"]``: T-GATE (``enable_tgate``) swept over gate steps.

The reference's registry has no such method; it is built like ``freeu``: one setting per entry of
``experiment_params.gate_step`` (a list of integers >= 1; ``null`` = T-GATE off, the plain pipeline), enabled across the whole
sweep of ``num_inference_steps``.  A gate at or past the step count of a run is the plain pipeline for that run.  The
scheduler is ``scheduler.scheduler_name`` where given, else the checkpoint's own."""
from ..registry import methods_registry, schedulers_registry
from ..schedulers import checkpoint_scheduler_name
from .base_experiment import BaseMethod


@methods_registry.add_to_registry("tgate")
class TGateMethod(BaseMethod):
    def setup_exp_params(self):
        ep = self.config.experiment_params
        settings = ep.gate_step
        if settings is None or isinstance(settings, (str, bytes)) or hasattr(settings, "keys") or not hasattr(settings, "__iter__"):
            raise ValueError("experiment_params.gate_step must be a list of integers >= 1 (null = off)")
        self.gate_steps = [self.parse_tgate({"tgate_step": g}) for g in settings]      # refused by name before any GPU work
        self.num_inference_steps = ep.num_inference_steps

    def setup_scheduler(self):
        config = self.model.scheduler.config
        name = self.config.get("scheduler", {}).get("scheduler_name", None) or checkpoint_scheduler_name(config)
        self.model.scheduler = schedulers_registry[name].from_config(config)

    def run_experiment(self):
        for g in self.gate_steps:
            label = "off" if g is None else str(g)
            if g is None:
                self.model.disable_tgate()
            else:
                self.model.enable_tgate(g)
            try:
                self.sweep(self.num_inference_steps, lambda n: {"num_inference_steps": n},
                           lambda n: f"Inference steps: {n}, T-GATE gate step: {label}",
                           extra=lambda n: {"T-GATE": label})
            finally:
                self.model.disable_tgate()
