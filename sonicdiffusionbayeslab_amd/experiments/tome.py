"""``methods_registry["tome"]``: Token Merging for Stable Diffusion (``tomesd.apply_patch``) swept over merge ratios.

The reference's registry has no such method; it is built like ``deep_cache``: one setting per entry of
``experiment_params.tome_ratio`` (a list), enabled across the whole sweep of ``num_inference_steps``.  The scheduler is
``scheduler.scheduler_name`` where given, else the checkpoint's own.  Optional ``experiment_params.tome_max_downsample``
(1 | 2), ``tome_use_rand`` and ``tome_seed``."""
from ..registry import methods_registry, schedulers_registry
from ..schedulers import checkpoint_scheduler_name
from .base_experiment import BaseMethod


@methods_registry.add_to_registry("tome")
class TomeMethod(BaseMethod):
    def setup_exp_params(self):
        ep = self.config.experiment_params
        ratios = ep.tome_ratio
        self.tome_ratio = [float(r) for r in (ratios if isinstance(ratios, (list, tuple)) or hasattr(ratios, "__iter__") else [ratios])]
        self.num_inference_steps = ep.num_inference_steps
        self.tome_max_downsample = int(ep.get("tome_max_downsample", 1))
        self.tome_use_rand = bool(ep.get("tome_use_rand", True))
        self.tome_seed = int(ep.get("tome_seed", 0))
        from ..models import StableDiffusionModel
        for r in self.tome_ratio:          # refused by name before any GPU work
            StableDiffusionModel.check_tome_args(ratio=r, max_downsample=self.tome_max_downsample)

    def setup_scheduler(self):
        config = self.model.scheduler.config
        name = self.config.get("scheduler", {}).get("scheduler_name", None) or checkpoint_scheduler_name(config)
        self.model.scheduler = schedulers_registry[name].from_config(config)

    def run_experiment(self):
        for ratio in self.tome_ratio:
            self.model.apply_tome(ratio=ratio, max_downsample=self.tome_max_downsample, use_rand=self.tome_use_rand,
                                  seed=self.tome_seed)
            try:
                self.sweep(self.num_inference_steps, lambda n: {"num_inference_steps": n},
                           lambda n: f"Inference steps: {n}, ToMe ratio: {ratio}",
                           extra=lambda n: {"ToMe ratio": ratio})
            finally:
                self.model.remove_tome()
