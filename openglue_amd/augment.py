"""weak_color_aug on HIP kernels: the photometric augmentation of the reference's online training step (models/matching_module.py:55-74
MatchingTrainingModule.augment, utils/augmentations.py get_augmentation_transform), which the reference runs with kornia on the GPU:
RandomEqualize(p=.25), RandomSharpness(p=.25), RandomSolarize(p=.25), RandomGaussianNoise(p=.5, std=.05), applied in that order to
image0 and to image1, every sample of the batch with its own draw.

  sample_weak_color_aug       the draw of a batch: four flags and the scalars of every sample, on the device
  color_aug                   the four operations on a batch of images, three launches (og_color_aug, csrc/coloraug.hip)
  get_augmentation_transform  the reference's factory: 'none' or 'weak_color_aug'
  augment                     MatchingTrainingModule.augment: replaces image0 / image1 of a batch

GPU tensors only, no host synchronisation.  The kernels are bit-identical to the numpy restatement in tests/coloraug_ref.py in everything
but the Gaussian noise (there: to the accuracy of logf / cosf), from run to run and whatever the batch.  What differs from kornia
(DESIGN.md 4.17): the random stream (torch.rand of one generator for the draw, a counter-based hash for the noise); the histogram is
counted in integers (kornia's float32 histogram stops being exact beyond 2^24 pixels); values outside [0, 1] are clamped into the first
and the last bin where kornia raises; images with a side below 3 pass the sharpness unchanged where kornia's conv2d raises.  All four
operations change intensities only: transform_matrix is None and K0 / K1 stay as they are.
"""
from __future__ import annotations

from typing import Any, Callable, Dict, Optional

import torch

from . import _lib
from .geometry import _shape
from .pairs import MAX_BATCH, MAX_HW

EQUALIZE, SHARPNESS, SOLARIZE, NOISE = 1, 2, 4, 8            # the bits of og_color_aug's flags
_FLAGS = ("equalize", "sharpness", "solarize", "noise")
_SCALARS = ("factor", "threshold", "addition", "noise_mean", "noise_std")      # the columns of og_color_aug's scalars


def sample_weak_color_aug(batch: int, device, generator=None, *, p_equalize=.25, p_sharpness=.25, sharpness=.5, p_solarize=.25, thresholds=.1,
                          additions=.1, p_noise=.5, noise_mean=0., noise_std=.05) -> Dict[str, torch.Tensor]:
    """The draw of kornia's four augmentations for `batch` samples, on `device` from `generator`, without a synchronisation:
    {'equalize', 'sharpness', 'solarize', 'noise': bool [batch] (probability p_*), 'factor' ~ U(0, sharpness), 'threshold' ~
    U(.5 - thresholds, .5 + thresholds), 'addition' ~ U(-additions, additions), 'noise_mean', 'noise_std': float32 [batch],
    'seed': int64 [batch] in [0, 2^63 - 1)}.  The defaults are kornia's and the probabilities utils/augmentations.py sets."""
    if isinstance(batch, bool) or not isinstance(batch, int) or not 0 < batch <= MAX_BATCH:
        raise ValueError(f"batch must be an int in [1, {MAX_BATCH}], got {batch!r}")
    p = [float(v) for v in (p_equalize, p_sharpness, p_solarize, p_noise)]
    if not all(0.0 <= v <= 1.0 for v in p):
        raise ValueError(f"the probabilities must lie in [0, 1], got {p}")
    dev = torch.device(device)
    u = torch.rand(7, batch, device=dev, generator=generator)                 # rows 0-3: the flags; 4-6: factor, threshold, addition
    out = {name: u[i] < p[i] for i, name in enumerate(_FLAGS)}
    out["factor"] = u[4] * float(sharpness)
    out["threshold"] = (0.5 - float(thresholds)) + u[5] * (2.0 * float(thresholds))
    out["addition"] = -float(additions) + u[6] * (2.0 * float(additions))
    out["noise_mean"] = torch.full((batch,), float(noise_mean), device=dev)
    out["noise_std"] = torch.full((batch,), float(noise_std), device=dev)
    out["seed"] = torch.randint(0, 2 ** 63 - 1, (batch,), device=dev, generator=generator)
    return out


def _check_params(params, B: int) -> None:
    if not isinstance(params, dict):
        raise ValueError("params must be the dictionary sample_weak_color_aug returns")
    for name, dtype in [(n, torch.bool) for n in _FLAGS] + [(n, torch.float32) for n in _SCALARS] + [("seed", torch.int64)]:
        if name not in params:
            raise ValueError(f"params lacks '{name}'")
        if _shape(params[name], name) != (B,) or params[name].dtype != dtype:
            raise ValueError(f"params['{name}'] must be {dtype} [B] = [{B}], got {params[name].dtype} {list(params[name].shape)}")


def pack_params(params) -> tuple:
    """-> (flags int32 [B], scalars float32 [B, 5], seeds int64 [B]): the three device tables of og_color_aug"""
    flags = params[_FLAGS[0]].to(torch.int32)
    for i in (1, 2, 3):
        flags.add_(params[_FLAGS[i]], alpha=1 << i)
    scalars = torch.stack([params[name] for name in _SCALARS], dim=1).contiguous()
    return flags, scalars, params["seed"].contiguous()


def color_aug_packed(image: torch.Tensor, flags: torch.Tensor, scalars: torch.Tensor, seeds: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """og_color_aug on a contiguous float32 GPU image [B, C, H, W] and the tables of pack_params; out: a contiguous tensor like image
    to write into (not image itself)"""
    B, C, H, W = image.shape
    if out is None:
        out = torch.empty_like(image)
    nbytes = _lib.load().og_color_aug_workspace_bytes(B, C, H, W)
    ws, ws_ptr = _lib.workspace(nbytes, image.device)
    _lib.call("og_color_aug", image.device, B, C, H, W, image.data_ptr(), out.data_ptr(), flags.data_ptr(), scalars.data_ptr(), seeds.data_ptr(),
              ws_ptr, nbytes, _lib.STREAM)
    return out


def color_aug(image, params) -> torch.Tensor:
    """image float32 [B, C, H, W], C in {1, 3}, nominally in [0, 1]; params: the dictionary of sample_weak_color_aug -> a new tensor of
    the same shape: equalize, sharpness, solarize and noise in that order, each on the samples whose flag is set."""
    s = _shape(image, "image")
    if len(s) != 4 or s[1] not in (1, 3):
        raise ValueError(f"image must be [B, C, H, W] with C in {{1, 3}}, got {list(s)}")
    if image.dtype != torch.float32:
        raise ValueError(f"image must be float32, got {image.dtype}")
    B, C, H, W = s
    if not (0 < B <= MAX_BATCH and 0 < H <= MAX_HW and 0 < W <= MAX_HW):
        raise ValueError(f"image {list(s)}: 0 < B <= {MAX_BATCH} and 0 < H, W <= {MAX_HW}")
    _check_params(params, B)
    img = _lib.gpu_tensor(image, "image").detach()
    for name in _FLAGS + _SCALARS + ("seed",):
        _lib.gpu_tensor(params[name], name, params[name].dtype)
    return color_aug_packed(img, *pack_params(params))


class _Transform:
    """what get_augmentation_transform returns: transform(image, generator=None) -> image; transform_matrix as kornia's
    AugmentationSequential has it, None here (intensity operations only)"""

    def __init__(self, name: str):
        self.name = name
        self.transform_matrix = None

    def __call__(self, image, generator=None):
        if self.name == "none":
            return image
        if not isinstance(image, torch.Tensor) or image.dim() != 4:
            raise ValueError("image must be a tensor [B, C, H, W]")
        return color_aug(image, sample_weak_color_aug(image.shape[0], image.device, generator))


def get_augmentation_transform(config) -> Callable:
    """utils/augmentations.py: config['name'] in 'none', 'weak_color_aug'"""
    method_name = config["name"]
    allowed_methods = ["none", "weak_color_aug"]
    if method_name not in allowed_methods:
        raise NameError("{} module was not found among local descriptors. Please choose one of the following "
                        "methods: {}".format(method_name, ", ".join(allowed_methods)))
    return _Transform(method_name)


@torch.no_grad()
def augment(batch: Dict[str, Any], transform, generator: Optional[torch.Generator] = None) -> Dict[str, Any]:
    """MatchingTrainingModule.augment: image0 and image1 of `batch` are replaced by their augmentations (each with its own draw);
    'transformation' is touched only where the transform reports a geometric matrix, which the colour augmentations never do."""
    image0 = transform(batch["image0"], generator)
    transform0 = transform.transform_matrix
    image1 = transform(batch["image1"], generator)
    transform1 = transform.transform_matrix
    batch["image0"], batch["image1"] = image0, image1
    tr = batch.get("transformation", {})
    if "K0" in tr and transform0 is not None:
        tr["K0"] = torch.matmul(transform0, tr["K0"])
    if "K1" in tr and transform1 is not None:
        tr["K1"] = torch.matmul(transform1, tr["K1"])
    return batch
