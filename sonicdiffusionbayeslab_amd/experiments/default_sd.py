"""``methods_registry["default"]`` (``src/experiments/default_sd.py:10-100``): the checkpoint's own
scheduler (never swapped: ``:15-16``; PNDM/PLMS for SD-1.5, else the class its scheduler config names) swept over
``num_inference_steps``."""
from ..registry import methods_registry, schedulers_registry
from ..schedulers import checkpoint_scheduler_name
from .base_experiment import BaseMethod


@methods_registry.add_to_registry("default")
class DefaultStableDiffusion(BaseMethod):
    def setup_exp_params(self):
        self.num_inference_steps = self.config.experiment_params.num_inference_steps

    def setup_scheduler(self):
        config = self.model.scheduler.config
        self.model.scheduler = schedulers_registry[checkpoint_scheduler_name(config)].from_config(config)

    def run_experiment(self):
        self.sweep(self.num_inference_steps, lambda n: {"num_inference_steps": n}, lambda n: f"Inference steps: {n}")
