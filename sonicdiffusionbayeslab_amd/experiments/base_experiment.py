"""Harness base class with the reference's hook order and benchmark semantics
(``src/experiments/base_experiment.py:18-163``): 7 ``setup_*`` hooks in fixed order, one shared
``torch.Generator`` that is never reseeded, scheduler swap through the registry +
``from_config``, ``generate()`` looping prompt batches through ``self.model(...)`` and feeding
``time_metric``.  Quality metrics that need fetched models and the wandb logger are out of the
hot-path scope; results go to stdout as JSON lines.

Multi-GPU (new relative to the single-device reference): launched under
``torch.distributed.run`` (one process per GPU), every prompt batch is split contiguously over the ranks,
each rank samples its shard on its own weight replica, and ONE all-gather per batch returns the results to
every rank.  Every Gaussian a pipeline call consumes (initial latents, LCM re-noising, SDE-DPM-Solver noise, eta > 0, the
variant pipelines' draws) is drawn for the GLOBAL batch from the shared seeded CPU generator, in the single-process order,
and sliced per rank (``dist.randn`` / ``dist.shard_draws``), so the inputs of every image are the same for every world
size -- also for the stochastic samplers, ragged shards and ranks without a prompt."""
from __future__ import annotations

import contextlib
import json
import os
from abc import ABC, abstractmethod
from collections import defaultdict

import torch

from .. import dist as sdist
from ..dataset import PromptDataset, load_image
from ..registry import metrics_registry, models_registry, schedulers_registry


class BaseMethod(ABC):
    def __init__(self, config):
        self.config = config
        # one process per GPU under torch.distributed.run (RANK / LOCAL_RANK / WORLD_SIZE); world 1 otherwise.
        # SD_DIST_BACKEND=gloo is the CPU-side rehearsal backend of the tests (ranks may then share one GPU)
        backend = os.environ.get("SD_DIST_BACKEND", "nccl" if torch.cuda.is_available() else "gloo")
        self.rank, local_rank, self.world = sdist.init_process_group(backend)
        ngpu = torch.cuda.device_count() if torch.cuda.is_available() else 0
        self.device = f"cuda:{local_rank % ngpu}" if ngpu else "cpu"
        if ngpu:
            torch.cuda.set_device(self.device)
        self.setup_exp_params()
        self.setup_generator()
        self.setup_model()
        self.setup_scheduler()
        self.setup_dataset()
        self.setup_metrics()
        self.setup_loggers()

    @abstractmethod
    def run_experiment(self):
        pass

    def setup_exp_params(self):
        pass

    def setup_generator(self):
        # the reference seeds a device generator (:51-53); a CPU generator makes the initial latents
        # identical for every world size and box
        self.generator = torch.Generator(device="cpu")
        self.generator.manual_seed(self.config.experiment.seed)

    def setup_model(self):
        model_name = self.config.model.model_name
        extra = {}
        if self.config.model.get("weight_dtype", None) is not None:      # key of this build: "bf16" | "fp8"
            extra["weight_dtype"] = self.config.model.weight_dtype
        if self.config.model.get("time_cond_proj_dim", None) is not None:   # key of this build: shapes a hub name's stand-in
            extra["time_cond_proj_dim"] = int(self.config.model.time_cond_proj_dim)
        for key in ("unet_arch", "sample_size", "prediction_type"):         # keys of this build: shape a hub name's stand-in ("sd2")
            if self.config.model.get(key, None) is not None:
                extra[key] = self.config.model[key]
        self.model = models_registry[model_name].from_pretrained(
            self.config.model.pretrained_model,
            timestamps=self.config.model.get("timestamps", None),
            safety_checker=None,
            requires_safety_checker=False,
            torch_dtype=torch.float16,
            **extra,
        )
        if self.config.model.get("controlnet", None) is not None:      # key of this build: a local ControlNet directory or a hub name
            self.model.load_controlnet(str(self.config.model.controlnet))
        if self.config.model.get("tiny_vae", None) is not None:        # key of this build: a local AutoencoderTiny directory or a hub name
            self.model.load_tiny_vae(str(self.config.model.tiny_vae), use_for=str(self.config.model.get("tiny_vae_use", "all")))
        tome = self.parse_tome(self.config.model)      # keys of this build: model.tome_ratio (+ tome_max_downsample, tome_use_rand, tome_seed)
        if tome is not None:
            self.model.apply_tome(**tome)
        freeu = self.parse_freeu(self.config.model, self.config.model.get("weight_dtype", None) or "bf16")     # key of this build: model.freeu
        if freeu is not None:
            self.model.enable_freeu(**freeu)
        hypertile = self.parse_hypertile(self.config.model, self.config.model.get("weight_dtype", None) or "bf16")    # key of this build: model.hypertile
        if hypertile is not None:
            self.model.enable_hypertile(**hypertile)
        pag = self.parse_pag(self.config.model, self.config.model.get("weight_dtype", None) or "bf16")    # key of this build: model.pag
        if pag is not None:
            self.model.enable_pag(**pag)
        sag = self.parse_sag(self.config.model, self.config.model.get("weight_dtype", None) or "bf16")    # key of this build: model.sag
        if sag is not None:
            self.model.enable_sag(**sag)
        gate = self.parse_tgate(self.config.model)     # key of this build: model.tgate_step
        if gate is not None:
            self.model.enable_tgate(gate)
        self.model.to(self.device)

    @staticmethod
    def parse_tgate(model_cfg):
        """``model.tgate_step`` -> the argument of ``enable_tgate`` (T-GATE for any method), or None when the key is absent or
        null.  Anything but an integer >= 1 is refused by name."""
        g = model_cfg.get("tgate_step", None)
        if g is None:
            return None
        from ..models import StableDiffusionModel
        return StableDiffusionModel.check_tgate_step(g)

    @staticmethod
    def parse_sag(model_cfg, weight_dtype="bf16"):
        """``model.sag: {scale}`` -> the arguments of ``enable_sag`` (self-attention guidance for any method), or None when the
        key is absent or null.  ``scale`` is optional (default 0.75); unknown keys, bad values and fp8 UNets are refused by
        name."""
        p = model_cfg.get("sag", None)
        if p is None:
            return None
        if not hasattr(p, "keys"):
            raise ValueError(f"model.sag must be a mapping {{scale}}, got {p!r}")
        keys = set(p.keys())
        if not keys <= {"scale"}:
            raise ValueError(f"model.sag takes the key scale (got {sorted(keys)})")
        from ..models import StableDiffusionModel
        out = dict(sag_scale=p.get("scale", 0.75))
        StableDiffusionModel.check_sag_args(out["sag_scale"], None, weight_dtype)
        return out

    @staticmethod
    def parse_pag(model_cfg, weight_dtype="bf16"):
        """``model.pag: {scale, adaptive_scale, applied_layers}`` -> the arguments of ``enable_pag`` (perturbed-attention
        guidance for any method), or None when the key is absent or null.  Every key is optional (defaults 3.0, 0.0, "mid");
        unknown keys, bad values and fp8 UNets are refused by name (the layer names are resolved when the model is built)."""
        p = model_cfg.get("pag", None)
        if p is None:
            return None
        if not hasattr(p, "keys"):
            raise ValueError(f"model.pag must be a mapping {{scale, adaptive_scale, applied_layers}}, got {p!r}")
        keys = set(p.keys())
        if not keys <= {"scale", "adaptive_scale", "applied_layers"}:
            raise ValueError(f"model.pag takes the keys scale, adaptive_scale and applied_layers (got {sorted(keys)})")
        from ..models import StableDiffusionModel
        layers = p.get("applied_layers", "mid")
        layers = layers if isinstance(layers, str) else list(layers)
        out = dict(pag_scale=p.get("scale", 3.0), pag_adaptive_scale=p.get("adaptive_scale", 0.0), pag_applied_layers=layers)
        StableDiffusionModel.check_pag_args(out["pag_scale"], out["pag_adaptive_scale"], layers, None, weight_dtype)
        if weight_dtype not in (None, "bf16"):
            from ..unet import HipUNet2DConditionModel
            from ..weights import UNetConfig
            HipUNet2DConditionModel.check_pag_handle(UNetConfig(), weight_dtype)
        return out

    @staticmethod
    def parse_hypertile(model_cfg, weight_dtype="bf16"):
        """``model.hypertile: {tile_size, max_depth}`` -> the arguments of ``enable_hypertile`` (HyperTile for any method), or
        None when the key is absent or null.  ``tile_size`` is required, ``max_depth`` defaults to 0; unknown keys, bad values
        and fp8 UNets are refused by name."""
        h = model_cfg.get("hypertile", None)
        if h is None:
            return None
        if not hasattr(h, "keys"):
            raise ValueError(f"model.hypertile must be a mapping {{tile_size, max_depth}}, got {h!r}")
        keys = set(h.keys())
        if "tile_size" not in keys or not keys <= {"tile_size", "max_depth"}:
            raise ValueError(f"model.hypertile takes the keys tile_size and (optionally) max_depth (got {sorted(keys)})")
        from ..models import StableDiffusionModel
        tile_size, max_depth = h["tile_size"], h.get("max_depth", 0)
        StableDiffusionModel.check_hypertile_args(tile_size, max_depth, 1, weight_dtype)
        return dict(tile_size=tile_size, max_depth=max_depth)

    @staticmethod
    def parse_freeu(model_cfg, weight_dtype="bf16"):
        """``model.freeu: {s1, s2, b1, b2}`` -> the arguments of ``enable_freeu`` (FreeU for any method), or None when the key
        is absent or null.  All four factors are required; unknown keys, factors <= 0 and fp8 UNets are refused by name."""
        f = model_cfg.get("freeu", None)
        if f is None:
            return None
        if not hasattr(f, "keys"):
            raise ValueError(f"model.freeu must be a mapping {{s1, s2, b1, b2}}, got {f!r}")
        keys = set(f.keys())
        if keys != {"s1", "s2", "b1", "b2"}:
            raise ValueError(f"model.freeu takes exactly the keys s1, s2, b1, b2 (got {sorted(keys)})")
        from ..models import StableDiffusionModel
        s1, s2, b1, b2 = StableDiffusionModel.check_freeu_args(f["s1"], f["s2"], f["b1"], f["b2"], weight_dtype)
        return dict(s1=s1, s2=s2, b1=b1, b2=b2)

    @staticmethod
    def parse_tome(model_cfg):
        """``model.tome_ratio`` / ``tome_max_downsample`` / ``tome_use_rand`` / ``tome_seed`` -> the arguments of
        ``apply_tome``, or None when ``tome_ratio`` is absent (Token Merging for any method)."""
        if model_cfg.get("tome_ratio", None) is None:
            for key in ("tome_max_downsample", "tome_use_rand", "tome_seed"):
                if model_cfg.get(key, None) is not None:
                    raise ValueError(f"model.{key} is set but model.tome_ratio is not")
            return None
        return dict(ratio=float(model_cfg.tome_ratio), max_downsample=int(model_cfg.get("tome_max_downsample", 1)),
                    use_rand=bool(model_cfg.get("tome_use_rand", True)), seed=int(model_cfg.get("tome_seed", 0)))

    def setup_scheduler(self, **kwargs):
        scheduler_name = self.config.scheduler.scheduler_name
        self.model.scheduler = schedulers_registry[scheduler_name].from_config(self.model.scheduler.config, **kwargs)

    def setup_dataset(self):
        self.test_dataset = PromptDataset(self.config.dataset.img_dataset, self.config.dataset.prompts)
        # optional experiment_params.strength (key of this build): image-to-image -- every prompt's own file from
        # dataset.img_dataset is the start image of its sample.  Absent: nothing is opened, as before.
        strength = self.config.get("experiment_params", {}).get("strength", None)
        self.img2img_strength = None if strength is None else float(strength)
        if self.img2img_strength is not None and not os.path.isdir(str(self.config.dataset.img_dataset)):
            raise FileNotFoundError(f"experiment_params.strength is set (image-to-image) but the image directory "
                                    f"dataset.img_dataset = {str(self.config.dataset.img_dataset)!r} does not exist")

        # optional experiment_params.inpaint_box = [top, left, bottom, right] (key of this build), pixels of dataset.image_size,
        # each a multiple of 8: inpainting -- every prompt's own file is the image and the box the region to repaint;
        # strength is experiment_params.strength, or 1.0.  Absent: nothing changes.
        self.inpaint_box = self.parse_inpaint_box(self.config.get("experiment_params", {}).get("inpaint_box", None),
                                                  int(self.config.dataset.get("image_size", 512)))
        if self.inpaint_box is not None:
            if not os.path.isdir(str(self.config.dataset.img_dataset)):
                raise FileNotFoundError(f"experiment_params.inpaint_box is set (inpainting) but the image directory "
                                        f"dataset.img_dataset = {str(self.config.dataset.img_dataset)!r} does not exist")
            if self.img2img_strength is None:
                self.img2img_strength = 1.0

        # optional experiment_params.control_from_dataset: true (key of this build): every prompt's own file is the control
        # image of its sample (model.controlnet), at experiment_params.controlnet_conditioning_scale (default 1.0)
        ep = self.config.get("experiment_params", {})
        self.control_from_dataset = bool(ep.get("control_from_dataset", False))
        self.controlnet_conditioning_scale = float(ep.get("controlnet_conditioning_scale", 1.0))
        if self.control_from_dataset:
            if self.config.model.get("controlnet", None) is None:
                raise ValueError("experiment_params.control_from_dataset is set but model.controlnet names no ControlNet")
            if self.inpaint_box is not None:
                raise NotImplementedError("experiment_params.control_from_dataset with inpaint_box (a ControlNet with inpainting) "
                                          "is not built")
            if not os.path.isdir(str(self.config.dataset.img_dataset)):
                raise FileNotFoundError(f"experiment_params.control_from_dataset is set but the image directory "
                                        f"dataset.img_dataset = {str(self.config.dataset.img_dataset)!r} does not exist")

    @staticmethod
    def parse_inpaint_box(box, image_size: int):
        """``experiment_params.inpaint_box`` -> (top, left, bottom, right) or None.  Four integers, multiples of 8, with
        0 <= top < bottom <= image_size and 0 <= left < right <= image_size; anything else raises ``ValueError``."""
        if box is None:
            return None
        box = list(box) if isinstance(box, (list, tuple)) else box
        if not isinstance(box, list) or len(box) != 4 or any(isinstance(v, bool) or not isinstance(v, int) for v in box):
            raise ValueError(f"experiment_params.inpaint_box={box!r}: four integers [top, left, bottom, right]")
        t, l, b, r = box
        if any(v % 8 for v in box) or not (0 <= t < b <= image_size and 0 <= l < r <= image_size):
            raise ValueError(f"experiment_params.inpaint_box={box!r}: multiples of 8 with 0 <= top < bottom <= {image_size} and "
                             f"0 <= left < right <= {image_size} (dataset.image_size)")
        return t, l, b, r

    def inpaint_mask(self, n: int) -> torch.Tensor:
        """The box as a mask [n, 1, S, S]: 1 inside (repaint), 0 outside (keep)."""
        size = int(self.config.dataset.get("image_size", 512))
        t, l, b, r = self.inpaint_box
        m = torch.zeros(n, 1, size, size)
        m[:, :, t:b, l:r] = 1.0
        return m

    def load_images(self, files):
        """The start images of one prompt batch, ``[B, 3, S, S]`` in [0, 1] (``dataset.image_size``; the reference's
        transform, ``dataset.image_transform``)."""
        size = int(self.config.dataset.get("image_size", 512))
        root = str(self.config.dataset.img_dataset)
        return torch.stack([load_image(os.path.join(root, f), size) for f in files])

    def setup_metrics(self):
        """``src/experiments/base_experiment.py:93-113``.  ``time_metric`` always; ``clip_score`` (``:96-98``) when
        ``quality_metrics.clip_score.model_name_or_path`` is a LOCAL checkpoint directory -- a hub name is a network
        fetch and the metric is then reported as not computable.  ``fid`` (``:105-109``) when the key of this
        build ``quality_metrics.fid.weights`` names a LOCAL Inception checkpoint file (beside the reference's ``feature`` /
        ``input_img_size`` / ``normalize``).  ``image_reward`` (``:99-104``) when the key of this build
        ``quality_metrics.image_reward.model_path`` names a LOCAL ImageReward directory (beside the reference's
        ``model_name``); the hub name alone is a network fetch."""
        self.metric_dict = defaultdict(list)
        self.time_metric = metrics_registry["time_metric"]()
        self.clip_score_gen_metric = None
        qm = self.config.get("quality_metrics", None)
        path = qm.get("clip_score", {}).get("model_name_or_path", None) if qm else None
        # optional quality_metrics.clip_score.backend ("transformers" | "hip"); absent: the metric's default
        backend = qm.get("clip_score", {}).get("backend", None) if qm else None
        if path and os.path.isdir(str(path)):
            kw = {"backend": str(backend)} if backend else {}
            if backend == "hip" and str(self.device).startswith("cuda"):
                kw["device"] = self.device          # this rank's GPU (the towers are built at the first score)
            self.clip_score_gen_metric = metrics_registry["clip_score"](model_name_or_path=str(path), **kw)
        self.clip_score_source = str(path) if self.clip_score_gen_metric is not None else (
            f"not computable offline ({path!r} is not a local directory)" if path else "not configured")
        self.fid_metric = None
        fq = qm.get("fid", None) if qm else None
        fw = fq.get("weights", None) if fq else None
        if fw and os.path.isfile(str(fw)):
            kw = {"device": self.device} if str(self.device).startswith("cuda") else {}
            self.fid_metric = metrics_registry["fid"](feature=int(fq.get("feature", 2048)),
                                                      input_img_size=fq.get("input_img_size", None),
                                                      normalize=bool(fq.get("normalize", False)), weights=str(fw), **kw)
        self.fid_source = str(fw) if self.fid_metric is not None else (
            f"not computable offline ({fw!r} is not a local file)" if fw else "not configured")
        self.image_reward_metric = None
        iq = qm.get("image_reward", None) if qm else None
        self.image_reward_configured = bool(iq)
        ip = iq.get("model_path", None) if iq else None
        if ip and os.path.isdir(str(ip)):
            kw = {"device": self.device} if str(self.device).startswith("cuda") else {}
            self.image_reward_metric = metrics_registry["image_reward"](
                model_name=str(iq.get("model_name", "ImageReward-v1.0")), model_path=str(ip), **kw)
        self.image_reward_source = str(ip) if self.image_reward_metric is not None else (
            f"not computable offline (model_path {ip!r} is not a local directory; "
            f"{iq.get('model_name', 'ImageReward-v1.0')!r} is a network fetch)" if iq else "not configured")

    def setup_loggers(self):
        self.logger = None

    def generate(self, test_dataloader, steps=None, batch_size: int = 1, guidance_scale: float = 7.5, **call_kwargs):
        """One pass over the prompt batches through ``self.model(...)`` (``base_experiment.py:122-163``).
        ``steps`` becomes ``num_inference_steps``; pipelines with other step arguments (the variant
        pipelines) receive theirs through ``call_kwargs``."""
        if steps is not None:
            call_kwargs["num_inference_steps"] = steps
        limit = self.config.inference.get("batch_count", None)
        out_type = self.config.inference.get("output_type", "pt")        # the reference hard-codes "pt" (:145)
        images, x0_preds = [], []
        self.last_prompts = []                                           # prompt of every returned image, in order
        self.last_image_files = []                                       # and its file under dataset.img_dataset
        for idx, batch in enumerate(test_dataloader):
            if limit is not None and idx >= limit:
                break
            prompts = list(batch["prompt"])
            self.last_prompts.extend(prompts)
            self.last_image_files.extend(batch.get("image_file", []))
            sharded = sdist.active()
            lo, hi = sdist.shard_range(len(prompts), self.rank, self.world) if sharded else (0, len(prompts))
            local_prompts = prompts[lo:hi]
            if sharded and (call_kwargs.get("ip_adapter_image") is not None or call_kwargs.get("ip_adapter_image_embeds") is not None):
                # an IP-Adapter image prompt given per prompt is sliced with the prompts, as image= is below
                call_kwargs = self.model.shard_ip_adapter_args(call_kwargs, lo, hi, len(prompts))
            if sharded and call_kwargs.get("control_image") is not None:
                call_kwargs = self.model.shard_control_args(call_kwargs, lo, hi, len(prompts))
            if getattr(self, "control_from_dataset", False) and len(local_prompts) > 0:
                # ControlNet: this rank's slice of the batch's files as control images, like the start images below
                call_kwargs = {**call_kwargs, "control_image": self.load_images(list(batch["image_file"])[lo:hi]),
                               "controlnet_conditioning_scale": self.controlnet_conditioning_scale}
            if getattr(self, "img2img_strength", None) is not None and len(local_prompts) > 0:
                # image-to-image: this rank's slice of the batch's start images rides with its slice of the prompts
                call_kwargs = {**call_kwargs, "image": self.load_images(list(batch["image_file"])[lo:hi]),
                               "strength": self.img2img_strength}
                if getattr(self, "inpaint_box", None) is not None:
                    call_kwargs["mask_image"] = self.inpaint_mask(hi - lo)
            if len(local_prompts) > 0:
                # every Gaussian of the call (initial latents, per-step noise of the stochastic samplers) is drawn for the
                # GLOBAL batch from the shared generator and sliced: dist.randn inside dist.shard_draws
                with (sdist.shard_draws(len(prompts), lo, hi) if sharded else contextlib.nullcontext()):
                    result, seconds, x0_preds = self.model(local_prompts, guidance_scale=guidance_scale,
                                                           generator=self.generator, output_type=out_type, **call_kwargs)
                local = result.images
            else:                       # more ranks than prompts in a ragged last batch
                local, seconds = self._empty_result(out_type, call_kwargs.get("height"), call_kwargs.get("width")), 0.0
            if sharded:                 # the ONE data-path collective; the slowest rank's loop time rides along (and, when a
                                        # rank had no prompt and therefore drew nothing, rank 0's generator state)
                local, seconds = sdist.gather_latents(local, self.world, len(prompts), seconds=seconds,
                                                      generator=self.generator)
            host = local.cpu()
            images.extend(host[i] for i in range(host.shape[0]))
            self.time_metric.update(seconds, batch_size)                 # configured size, as :161
        return images, x0_preds

    def _empty_result(self, out_type: str, height=None, width=None) -> torch.Tensor:
        """What a rank without a prompt hands to the all-gather: no rows, at the size of the call the other ranks ran
        (``height`` / ``width`` in pixels as the call got them; None = the UNet's ``sample_size``) -- every rank must enter
        the collective with the same row size."""
        ucfg = self.model.unet_config
        h = ucfg.sample_size * 8 if height is None else int(height)
        w = ucfg.sample_size * 8 if width is None else int(width)
        if out_type == "latent":
            return torch.empty((0, ucfg.out_channels, h // 8, w // 8), device=self.device)
        return torch.empty((0, 3, h, w), device=self.device)

    def sweep(self, points, call_kwargs, label, extra=None, guidance_scale: float = 7.5):
        """The loop every method's ``run_experiment`` is: for each sweep point move the model to the device,
        generate, move it back, report (``src/experiments/ddim.py:26-57`` and its siblings).
        ``call_kwargs(point)`` -> keyword arguments of the pipeline call, ``label(point)`` -> run name,
        ``extra(point)`` -> additional logged values."""
        batch_size = self.config.inference.get("batch_size", 1)
        self.metric_dict = defaultdict(list)
        # optional experiment_params.guidance_rescale (rescaled CFG, src/models.py:244-250); absent: the call is unchanged
        rescale = self.config.get("experiment_params", {}).get("guidance_rescale", None)
        if rescale is not None:
            call_kwargs = (lambda kw: lambda p: {**kw(p), "guidance_rescale": float(rescale)})(call_kwargs)
        for point in points:
            self.model.to(self.device)
            if hasattr(self.model, "calibrate_fp8") and not getattr(self.model, "_fp8_calibrated", True):
                self.model.calibrate_fp8()      # fp8 handles: an explicit set-up step on EVERY rank (also one whose shards are empty)
            images, _ = self.generate(self.test_dataset.batches(batch_size), None, batch_size,
                                      guidance_scale=guidance_scale, **call_kwargs(point))
            self.model.to("cpu")
            self.validate(f"{self.config.experiment_name}, {label(point)}",
                          additional_values=extra(point) if extra else None, n_images=len(images),
                          images=images, prompts=self.last_prompts, image_files=getattr(self, "last_image_files", None))

    def clip_score(self, images, prompts, batch_size: int = 32):
        """``validate`` of the reference for the parity metric (``:198-201``): generated images -> uint8 by
        ``(img * 255).to(uint8)`` (truncation), CLIPScore over (image, prompt) pairs.  None when no local CLIP
        checkpoint was configured or the run produced latents."""
        m = self.clip_score_gen_metric
        if m is None or not images or images[0].dim() != 3 or images[0].shape[0] != 3:
            return None
        m.reset()
        for s in range(0, len(images), batch_size):
            gen = (torch.stack(images[s:s + batch_size]) * 255).to(torch.uint8).cpu()
            m.update(gen, prompts[s:s + batch_size])
        return float(m.compute())

    def fid(self, images, image_files, batch_size: int = 32):
        """``validate`` of the reference for FID (``:198-206``): per batch the generated images
        (``(img * 255).to(uint8)``, ``real=False``) and the dataset's images of the same files (``load_images``,
        ``real=True``).  None when no local Inception checkpoint was configured, the run produced latents, or a file of the
        batch is not under ``dataset.img_dataset``."""
        m = self.fid_metric
        if m is None or not images or images[0].dim() != 3 or images[0].shape[0] != 3:
            return None
        root = str(self.config.dataset.img_dataset)
        if not image_files or len(image_files) != len(images) or not all(os.path.isfile(os.path.join(root, f)) for f in image_files):
            self.fid_source = f"not computable: the batch's image files are not under dataset.img_dataset = {root!r}"
            return None
        m.reset()
        for s in range(0, len(images), batch_size):
            m.update((torch.stack(images[s:s + batch_size]) * 255).to(torch.uint8), real=False)
            m.update((self.load_images(image_files[s:s + batch_size]) * 255).to(torch.uint8), real=True)
        return float(m.compute())

    def image_reward(self, images, prompts, image_files, batch_size: int = 32):
        """``validate`` of the reference for ImageReward (``:198-206,249``): per batch the dataset's images of the batch's
        files (real) and the generated images, both ``(img * 255).to(uint8)``, with the prompts -> the win rate of the
        generated image.  None when no local ImageReward directory was configured, the run produced latents, or a file of
        the batch is not under ``dataset.img_dataset``."""
        m = self.image_reward_metric
        if m is None or not images or images[0].dim() != 3 or images[0].shape[0] != 3:
            return None
        root = str(self.config.dataset.img_dataset)
        if (not image_files or len(image_files) != len(images) or not prompts or len(prompts) != len(images) or
                not all(os.path.isfile(os.path.join(root, f)) for f in image_files)):
            self.image_reward_source = f"not computable: the batch's image files are not under dataset.img_dataset = {root!r}"
            return None
        m.reset()
        for s in range(0, len(images), batch_size):
            gen = (torch.stack(images[s:s + batch_size]) * 255).to(torch.uint8)
            real = (self.load_images(image_files[s:s + batch_size]) * 255).to(torch.uint8)
            m.update(real, gen, prompts[s:s + batch_size])
        return float(m.compute())

    def validate(self, name_images, additional_values=None, n_images=0, images=None, prompts=None, image_files=None):
        """The hot-path metric, seconds / image over the loop (``time_metric``), and -- with a local CLIP checkpoint and
        decoded images -- the reference's parity metric ``clip_score``; with a local Inception checkpoint and the batch's
        dataset images, ``fid`` and, with a local ImageReward directory, the ``image_reward`` win rate."""
        if additional_values:
            for k, v in additional_values.items():
                self.metric_dict[k].append(v)
        cs = self.clip_score(images, prompts) if (images is not None and self.rank == 0) else None
        if cs is not None:
            self.metric_dict["clip_score"].append(cs)
        fid = self.fid(images, image_files) if (images is not None and self.rank == 0) else None
        if fid is not None:
            self.metric_dict["fid"].append(fid)
        ir = self.image_reward(images, prompts, image_files) if (images is not None and self.rank == 0) else None
        if ir is not None:
            self.metric_dict["image_reward"].append(ir)
        t = float(self.time_metric.compute())
        self.metric_dict["nfe"].append(self.model.num_timesteps)
        self.metric_dict["time_metric"].append(t)
        self.time_metric.reset()
        if self.rank != 0:
            return
        line = {"experiment": self.config.experiment_name, "run": name_images, "nfe": self.model.num_timesteps,
                "images": n_images, "time_metric_s_per_image": t,
                "images_per_s": (1.0 / t if t > 0 else None), "weights": self.model.weights_source,
                "clip_score": cs, "clip_score_model": self.clip_score_source, "n_gpus": self.world,
                "fp8_activation_scales": self._fp8_scale_report(),
                "fid": fid, "fid_weights": self.fid_source}
        if getattr(self, "image_reward_configured", False):      # (a config without the key reports exactly what it did before)
            line.update({"image_reward": ir, "image_reward_model": self.image_reward_source})
        print(json.dumps(line), flush=True)

    def _fp8_scale_report(self):
        """The e4m3 activation scales the run used (fp8 handles; None otherwise): count, range and a digest, so that two
        runs -- or two world sizes -- can be checked to have quantised identically."""
        sc = getattr(self.model, "fp8_scales", None)
        if not sc:
            return None
        import hashlib
        digest = hashlib.sha256(json.dumps(sorted(sc.items())).encode()).hexdigest()[:16]
        return {"tensors": len(sc), "min": min(sc.values()), "max": max(sc.values()), "sha256_16": digest}
