"""``methods_registry["unipc"]``: UniPC (``UniPCScheduler``) swept over the number of inference steps, built like
``dpm_solver``.  ``experiment_params``: ``solver_order`` and ``num_inference_steps``; optional ``solver_type``,
``predict_x0``, ``disable_corrector``, ``use_karras_sigmas`` and ``final_sigmas_type`` (absent: the scheduler's defaults)."""
from ..registry import methods_registry
from .base_experiment import BaseMethod

OPTIONAL_KEYS = ("solver_type", "predict_x0", "disable_corrector", "use_karras_sigmas", "final_sigmas_type")


@methods_registry.add_to_registry("unipc")
class UniPCMethod(BaseMethod):
    def setup_exp_params(self):
        ep = self.config.experiment_params
        self.num_inference_steps = ep.num_inference_steps
        self.solver_order = ep.solver_order
        self.scheduler_kwargs = {}
        for k in OPTIONAL_KEYS:
            v = ep.get(k, None)
            if v is not None:
                self.scheduler_kwargs[k] = list(v) if k == "disable_corrector" else v

    def setup_scheduler(self, **kwargs):
        return super().setup_scheduler(solver_order=self.solver_order, **self.scheduler_kwargs)

    def run_experiment(self):
        self.sweep(self.num_inference_steps, lambda n: {"num_inference_steps": n},
                   lambda n: f"UniPC order: {self.solver_order}, Inference steps: {n}")
