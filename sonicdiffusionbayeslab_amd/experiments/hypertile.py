"""``methods_registry["hypertile"]``: HyperTile (tiled self-attention) swept over tile sizes.

The reference's registry has no such method; it is built like ``freeu``: one setting per entry of
``experiment_params.hypertile_tile_size`` (a list of tile sizes in pixels; ``null`` = HyperTile off, the plain pipeline),
enabled across the whole sweep of ``num_inference_steps``.  Optional ``experiment_params.hypertile_max_depth`` (0 .. 3,
default 0) and ``experiment_params.height`` / ``width`` (pixels; absent = the checkpoint's own size).  The scheduler is
``scheduler.scheduler_name`` where given, else the checkpoint's own."""
from ..models import StableDiffusionModel
from ..registry import methods_registry, schedulers_registry
from ..schedulers import checkpoint_scheduler_name
from .base_experiment import BaseMethod


@methods_registry.add_to_registry("hypertile")
class HyperTileMethod(BaseMethod):
    def setup_exp_params(self):
        ep = self.config.experiment_params
        sizes = ep.hypertile_tile_size
        if sizes is None or isinstance(sizes, (str, bytes)) or hasattr(sizes, "keys") or not hasattr(sizes, "__iter__"):
            raise ValueError("experiment_params.hypertile_tile_size must be a list of tile sizes in pixels (null = off)")
        self.hypertile_tile_size = list(sizes)
        self.hypertile_max_depth = ep.get("hypertile_max_depth", 0)
        weight_dtype = self.config.model.get("weight_dtype", None) or "bf16"
        for s in self.hypertile_tile_size:          # refused by name before any GPU work
            if s is not None:
                StableDiffusionModel.check_hypertile_args(s, self.hypertile_max_depth, 1, weight_dtype)
        self.size_kwargs = {k: int(ep[k]) for k in ("height", "width") if ep.get(k, None) is not None}
        self.num_inference_steps = ep.num_inference_steps

    def setup_scheduler(self):
        config = self.model.scheduler.config
        name = self.config.get("scheduler", {}).get("scheduler_name", None) or checkpoint_scheduler_name(config)
        self.model.scheduler = schedulers_registry[name].from_config(config)

    def run_experiment(self):
        for s in self.hypertile_tile_size:
            label = "off" if s is None else f"{s} px, max_depth {self.hypertile_max_depth}"
            if s is None:
                self.model.disable_hypertile()
            else:
                self.model.enable_hypertile(tile_size=s, max_depth=self.hypertile_max_depth)
            try:
                self.sweep(self.num_inference_steps, lambda n: {"num_inference_steps": n, **self.size_kwargs},
                           lambda n: f"Inference steps: {n}, HyperTile: {label}",
                           extra=lambda n: {"HyperTile": label})
            finally:
                self.model.disable_hypertile()
