"""Metric plugins.  ``time_metric`` keeps the reference's definition of speed
(``src/metrics/metrics.py:115-131``): sum(loop seconds) / sum(batch_size) -> seconds per image.
``clip_score`` is the reference's parity metric (``:25-41``, ``calc_clip_score.py:13-37``); it
needs CLIP ViT-B/16 weights that only exist as a network fetch, so it is registered but raises
unless a LOCAL checkpoint directory is given.  ``BaseMethod.setup_metrics`` builds it when
``quality_metrics.clip_score.model_name_or_path`` is such a directory and ``validate`` then reports it
(``src/experiments/base_experiment.py:96-98,198-201``).  ``fid`` (``:98-112``) runs the FID Inception-v3 on libsdhip from a
LOCAL checkpoint file (``quality_metrics.fid.weights``); there is no host network behind it.  ``image_reward``
(``:44-95``) is the ImageReward-v1.0 win rate of the generated image over the dataset's real one, on libsdhip from a LOCAL
model directory (``quality_metrics.image_reward.model_path``)."""
from __future__ import annotations

import os

import torch

from .registry import metrics_registry


@metrics_registry.add_to_registry("time_metric")
class TimeMetric:
    def __init__(self):
        self.reset()

    def update(self, time: float, batch_size: int) -> None:
        self.time += float(time)
        self.total += int(batch_size)

    def compute(self):
        return torch.tensor(self.time / self.total if self.total else float("nan"))

    def reset(self) -> None:
        self.time = 0.0
        self.total = 0


@metrics_registry.add_to_registry("clip_score")
class ClipScoreMetric:
    """100 * cos(E_img, E_txt), clamped at 0, averaged (torchmetrics 1.6.1 CLIPScore, A.8)."""

    def __init__(self, model_name_or_path: str = "openai/clip-vit-base-patch16", backend: str = "transformers",
                 device=None):
        """backend ``"transformers"``: CLIPModel + CLIPProcessor in fp32 on the host; ``"hip"``: both towers on libsdhip
        (``clip_score.HipClipScorer``, uint8 images in) on ``device`` (``None``: the current device when the towers are
        built).  The hip backend checks the checkpoint's config here and builds the towers at the first ``update``, so
        that a process that never scores (a rank other than 0) puts no CLIP weights on a GPU."""
        if backend not in ("transformers", "hip"):
            raise ValueError(f"clip_score backend {backend!r}: 'transformers' or 'hip'")
        if not os.path.isdir(str(model_name_or_path)):
            raise FileNotFoundError(
                f"CLIP checkpoint {model_name_or_path!r} is a network fetch and unavailable offline; "
                "pass a local directory to compute CLIP score")
        self.backend = backend
        if backend == "hip":
            from .clip_score import read_clip_configs
            read_clip_configs(str(model_name_or_path))          # unsupported configs fail here, before any GPU work
            self.path, self.device, self.scorer = str(model_name_or_path), device, None
            self.reset()
            return
        from transformers import CLIPModel, CLIPProcessor
        self.model = CLIPModel.from_pretrained(model_name_or_path).eval()
        self.processor = CLIPProcessor.from_pretrained(model_name_or_path)
        self.reset()

    @torch.no_grad()
    def update(self, images, text):
        if self.backend == "hip":
            if self.scorer is None:
                from .clip_score import HipClipScorer
                self.scorer = HipClipScorer.from_pretrained(self.path, device=self.device)
            _, score = self.scorer.score_pairs(images, list(text))
            self.score += score.sum().item()
            self.n += len(text)
            return
        inp = self.processor(text=list(text), images=[i for i in images], return_tensors="pt", padding=True, truncation=True)
        # (transformers 4.48 returns the projected embedding itself, 5.x an output object whose pooler_output is it)
        emb = lambda o: o if torch.is_tensor(o) else o.pooler_output
        img = emb(self.model.get_image_features(pixel_values=inp["pixel_values"]))
        txt = emb(self.model.get_text_features(input_ids=inp["input_ids"], attention_mask=inp["attention_mask"]))
        img = img / img.norm(p=2, dim=-1, keepdim=True)
        txt = txt / txt.norm(p=2, dim=-1, keepdim=True)
        self.score += (100 * (img * txt).sum(-1)).clamp(min=0).sum().item()
        self.n += len(text)

    def compute(self):
        return torch.tensor(self.score / max(self.n, 1))

    def reset(self):
        self.score, self.n = 0.0, 0


@metrics_registry.add_to_registry("fid")
class FID:
    """torchmetrics' ``FrechetInceptionDistance`` surface (the reference's ``FID``, ``src/metrics/metrics.py:98-112``) on
    libsdhip: Inception features on the GPU (``fid.HipInceptionFeatures``), the fp64 sum / outer-product sum / count per
    side on the GPU (``sd_fid_accumulate``), the Frechet distance on the host in fp64."""

    def __init__(self, feature: int = 2048, input_img_size=None, normalize: bool = False, reset_real_features: bool = True,
                 weights=None, device=None):
        """``weights``: a LOCAL ``.pth`` / ``.safetensors`` state dict of the FID Inception-v3 (pt_inception-2015-12-05).
        ``input_img_size`` is accepted and ignored (upstream sizes a dummy input with it).  The network is built at the first
        ``update``, so a process that never scores puts no weights on a GPU."""
        from .fid import check_feature
        self.feature = check_feature(feature)
        if not isinstance(normalize, bool):
            raise ValueError("Argument `normalize` expected to be a bool")
        if not isinstance(reset_real_features, bool):
            raise ValueError("Argument `reset_real_features` expected to be a bool")
        if weights is None or not os.path.isfile(str(weights)):
            raise FileNotFoundError(
                f"FID Inception weights {weights!r} are a network fetch and unavailable offline; "
                "pass a local checkpoint file to compute FID")
        self.weights, self.device = str(weights), device
        self.normalize, self.reset_real_features = normalize, reset_real_features
        self.feature_fn = None              # images uint8 [B,3,H,W] -> features [B, feature]; built at the first update
        self._state = {}
        self.reset(_all=True)

    def _side(self, real: bool, like: torch.Tensor):
        key = "real" if real else "fake"
        if self._state.get(key) is None:
            d = self.feature
            self._state[key] = (torch.zeros(d, dtype=torch.float64, device=like.device),
                                torch.zeros(d, d, dtype=torch.float64, device=like.device),
                                torch.zeros(1, dtype=torch.int64, device=like.device))
        return self._state[key]

    @torch.no_grad()
    def update(self, imgs: torch.Tensor, real: bool) -> None:
        if imgs.dim() == 3:
            imgs = imgs.unsqueeze(0)
        if self.normalize:
            if not imgs.is_floating_point():
                raise ValueError("normalize=True expects float images in [0, 1]")
            imgs = (imgs * 255).byte()
        if imgs.dtype != torch.uint8:
            raise ValueError(f"FID expects uint8 images (or float in [0, 1] with normalize=True), got {imgs.dtype}")
        if self.feature_fn is None:
            from .fid import HipInceptionFeatures
            net = HipInceptionFeatures.from_file(self.weights, device=self.device)
            self.feature_fn = lambda x: net.features(x, self.feature)
        f = self.feature_fn(imgs)
        total, cov, n = self._side(real, f)
        if f.is_cuda:
            from .fid import fid_accumulate
            fid_accumulate(f, total, cov, n)
        else:                               # features handed in on the host (a test's stand-in feature function)
            fd = f.double()
            total += fd.sum(0)
            cov += fd.t() @ fd
            n += fd.shape[0]

    def compute(self) -> torch.Tensor:
        from .fid import frechet_distance
        stats = []
        for key in ("real", "fake"):
            st = self._state.get(key)
            n = int(st[2].item()) if st is not None else 0
            if n < 2:
                raise RuntimeError("More than one sample is required for both the real and fake distributed to compute FID")
            total, cov = st[0].cpu(), st[1].cpu()
            mean = total / n
            stats.append((mean, (cov - n * torch.outer(mean, mean)) / (n - 1)))
        (mu_r, s_r), (mu_f, s_f) = stats
        return frechet_distance(mu_r, s_r, mu_f, s_f)

    def reset(self, _all: bool = False) -> None:
        """Forget the generated statistics, and the real ones unless ``reset_real_features=False``."""
        self._state["fake"] = None
        if _all or self.reset_real_features:
            self._state["real"] = None

    def calc_metric(self, imgs, reals) -> float:
        """``src/metrics/metrics.py:100-112``: PIL images (or uint8 ``[3,H,W]`` tensors) with a real / generated flag each."""
        import numpy as np
        for img, real in zip(imgs, reals):
            if not torch.is_tensor(img):
                img = torch.from_numpy(np.asarray(img.convert("RGB"), dtype=np.uint8).copy()).permute(2, 0, 1).contiguous()
            self.update(imgs=img, real=real)
        return self.compute().item()


@metrics_registry.add_to_registry("image_reward")
class RewardModel:
    """The reference's ``RewardModel`` (``src/metrics/metrics.py:44-95``): ImageReward-v1.0 scores the dataset's real image and
    the generated one against the prompt; the metric is the share of prompts whose generated image scores at least as high."""

    def __init__(self, model_name: str = "ImageReward-v1.0", device=None, model_path=None):
        """``model_path``: a LOCAL directory with ``ImageReward.pt`` (or ``.safetensors``), ``med_config.json`` and
        ``vocab.txt``; upstream's ``RM.load(model_name)`` is a hub download.  The config is checked here, the model is built
        on ``device`` (``None``: the current device) at the first ``update``, so a process that never scores puts no weights
        on a GPU."""
        if model_path is None or not os.path.isdir(str(model_path)):
            raise FileNotFoundError(
                f"ImageReward checkpoint {model_name!r} (model_path={model_path!r}) is a network fetch and unavailable offline; "
                "pass a local directory to compute the ImageReward win rate")
        from .image_reward import read_image_reward_dir
        read_image_reward_dir(str(model_path))                  # unsupported configs fail here, before any GPU work
        self.model_name, self.path, self.device, self.model = model_name, str(model_path), device, None
        self.reset()

    def _scorer(self):
        if self.model is None:
            from .image_reward import HipImageReward
            self.model = HipImageReward.from_pretrained(self.path, device=self.device)
        return self.model

    @torch.no_grad()
    def update(self, real_imgs, gen_imgs, prompts) -> None:
        """uint8 images (``[B,3,H,W]`` or lists of ``[3,H,W]``), one prompt per pair.  A tie is a win, as in the reference
        (``reward_real <= reward_gen``)."""
        prompts = list(prompts)
        m = self._scorer()
        real = m.score(prompts, real_imgs)
        gen = m.score(prompts, gen_imgs)
        self.wins += int((real <= gen).sum().item())
        self.total += len(prompts)

    def compute(self):
        return torch.tensor(self.wins / self.total if self.total else float("nan"))

    def reset(self) -> None:
        self.wins, self.total = 0, 0

    @torch.no_grad()
    def calc_metric(self, imgs, prompts) -> float:
        """Mean reward of ``imgs`` under their prompts.  DEVIATION: the reference's line (``src/metrics/metrics.py:87``)
        unpacks the list of rewards that ``score`` returns into two names and cannot run as written; the mean of the
        rewards is what its caller reports."""
        return float(self._scorer().score(list(prompts), imgs).double().mean().item())
