"""Homography training pairs on HIP kernels: the first stage of the reference's recipe, self-supervised homography pre-training
(pretrain_homography.py, config/homography_pretraining.yaml), whose samples the reference synthesises with cv2 in its data-loader
workers (data/oxford_paris_dataset.py:27-66 OxfordParis1MDataset.__getitem__, data/megadepth_dataset.py:33-52
MegaDepthWarpingDataset.__getitem__).  Here a batch of decoded frames becomes the pair and its homography without leaving the GPU.

  get_perspective_transform   cv2.getPerspectiveTransform, batched
  warp_perspective            cv2.warpPerspective (bilinear, constant border 0) on uint8, restricted to a destination window
  homography_pairs            the Oxford-Paris item for a whole batch: {'image0', 'image1', 'transformation'} as after the default collate
  warping_pairs               the MegaDepth-warping item for a whole batch

Thin wrappers over og_perspective_transform / og_warp_perspective_u8 / og_homography_pairs (include/openglue_amd.h, csrc/pairs.hip);
GPU tensors only, no host synchronisation.  The warp follows cv2's fixed-point scheme -- source coordinates rounded to 1/32 pixel,
integer bilinear weights that sum to 2^15 -- and the kernels are bit-identical to the numpy restatement in tests/pairs_ref.py, from
run to run and whatever the batch.  cv2 itself evaluates the coordinates block-wise, so its last bit can differ.

Out of scope: JPEG decoding and cv2.resize(..., INTER_AREA) to `resize_shape` are the loader's job, frames arrive as uint8 tensors;
the albumentations colour augmentation of oxford_paris_dataset.py:18-22 is not applied, so homography_pairs equals the reference
with that augmentation's probabilities at 0.  kornia's weak_color_aug of the training step is openglue_amd.augment.
"""
from __future__ import annotations

from typing import Any, Dict, Optional, Tuple

import torch

from . import _lib
from .geometry import _shape

MAX_BATCH, MAX_HW = 65535, 32768


def get_perspective_transform(src, dst) -> torch.Tensor:
    """src, dst [B, 4, 2] -> M [B, 3, 3] float64 with M (x, y, 1) ~ (u, v, 1) for the four point pairs, M[2][2] = 1; M = 0 for a
    singular system (three collinear points)."""
    s, d = _shape(src, "src"), _shape(dst, "dst")
    if len(s) != 3 or s[1:] != (4, 2) or d != s or not 0 < s[0] <= MAX_BATCH:
        raise ValueError(f"src / dst must both be [B, 4, 2] with 0 < B <= {MAX_BATCH}, got {list(s)} / {list(d)}")
    a = _lib.gpu_tensor(src, "src", convert=True)
    b = _lib.gpu_tensor(dst, "dst", convert=True)
    M = torch.empty(s[0], 3, 3, device=a.device, dtype=torch.float64)
    _lib.call("og_perspective_transform", a.device, s[0], a.data_ptr(), b.data_ptr(), M.data_ptr(), _lib.STREAM)
    return M


def _frames(images, name: str, channels=(1, 3)) -> Tuple[int, int, int, int]:
    """(B, H, W, C) of a uint8 frame batch [B, H, W] or [B, H, W, C]"""
    s = _shape(images, name)
    if images.dtype != torch.uint8:
        raise ValueError(f"{name} must be uint8, got {images.dtype}")
    if len(s) == 3:
        s = s + (1,)
    if len(s) != 4 or s[3] not in channels:
        raise ValueError(f"{name} must be [B, H, W] or [B, H, W, C] with C in {set(channels)}, got {list(images.shape)}")
    B, H, W, C = s
    if not (0 < B <= MAX_BATCH and 0 < H <= MAX_HW and 0 < W <= MAX_HW):
        raise ValueError(f"{name} {list(images.shape)}: 0 < B <= {MAX_BATCH} and 0 < H, W <= {MAX_HW}")
    return B, H, W, C


def warp_perspective(images, M, dsize: Optional[Tuple[int, int]] = None, origin: Tuple[int, int] = (0, 0)) -> torch.Tensor:
    """cv2.warpPerspective(images[b], M[b], (W, H)) with the defaults -- bilinear, constant border 0, M maps source to destination --
    of which only the window with `origin` (x0, y0) and `dsize` (w, h) (cv2's order; default: up to the frame's far corner) is
    computed.  images uint8 [B, H, W], [B, H, W, 1] or [B, H, W, 3]; M [B, 3, 3] -> uint8 [B, h, w] or [B, h, w, C]."""
    B, H, W, C = _frames(images, "images")
    if _shape(M, "M") != (B, 3, 3):
        raise ValueError(f"M must be [B, 3, 3] = [{B}, 3, 3], got {list(M.shape)}")
    x0, y0 = (int(v) for v in origin)
    w, h = (W - x0, H - y0) if dsize is None else (int(v) for v in dsize)
    if w < 1 or h < 1 or x0 < 0 or y0 < 0 or x0 + w > W or y0 + h > H:
        raise ValueError(f"the window origin ({x0}, {y0}) size {w} x {h} must lie inside the {W} x {H} frame")
    src = _lib.gpu_tensor(images, "images", torch.uint8)
    m = _lib.gpu_tensor(M, "M", torch.float64, convert=True)
    out = torch.empty((B, h, w) if images.dim() == 3 else (B, h, w, C), device=src.device, dtype=torch.uint8)
    _lib.call("og_warp_perspective_u8", src.device, B, H, W, C, src.data_ptr(), m.data_ptr(), x0, y0, w, h, out.data_ptr(), _lib.STREAM)
    return out


def _draw(B: int, bound: int, dev, generator) -> torch.Tensor:
    """np.random.randint(-bound, bound, size=(4, 2)) per pair, on the device: integers in [-bound, bound)"""
    if bound < 1:
        raise ValueError(f"random warp offsets need a positive bound, got {bound}; pass warp_offset")
    return torch.randint(-bound, bound, (B, 4, 2), device=dev, generator=generator).to(torch.float32)


def _offsets(warp_offset, B: int) -> None:
    if _shape(warp_offset, "warp_offset") != (B, 4, 2):
        raise ValueError(f"warp_offset must be [B, 4, 2] = [{B}, 4, 2], got {list(warp_offset.shape)}")


def _pairs(frames: torch.Tensor, B, H, W, C, offset, warp_offset, M):
    """og_homography_pairs: solve from warp_offset (M None), or warp with the matrices M"""
    f = _lib.gpu_tensor(frames, "frames", torch.uint8)
    dev = f.device
    h, w = H - 2 * offset, W - 2 * offset
    image0 = torch.empty(B, 1, h, w, device=dev, dtype=torch.float32)
    image1 = torch.empty(B, 1, h, w, device=dev, dtype=torch.float32)
    if M is None:
        wo = _lib.gpu_tensor(warp_offset, "warp_offset", convert=True)
        M = torch.empty(B, 3, 3, device=dev, dtype=torch.float64)
        Ht = torch.empty(B, 3, 3, device=dev, dtype=torch.float32)
    else:
        wo, Ht = None, None
    _lib.call("og_homography_pairs", dev, B, H, W, C, f.data_ptr(), offset, _lib.ptr(wo), image0.data_ptr(), image1.data_ptr(), _lib.ptr(Ht),
              M.data_ptr(), _lib.STREAM)
    return image0, image1, Ht


def _item(image0, image1, Hm) -> Dict[str, Any]:
    return {"image0": image0, "image1": image1, "transformation": {"type": ["perspective"] * Hm.shape[0], "H": Hm}}


def homography_pairs(frames, offset: int, warp_offset=None, generator=None) -> Dict[str, Any]:
    """The Oxford-Paris item for a batch.  frames uint8 [B, H, W, 3] (RGB), [B, H, W, 1] or [B, H, W]; offset: the margin cut from
    every side and the bound of the corner displacements -> {'image0', 'image1': float32 [B, 1, H - 2 offset, W - 2 offset] in [0, 1],
    'transformation': {'type': ['perspective'] * B, 'H': float32 [B, 3, 3]}} with H mapping pixels of image0 to image1;
    supervision.generate_gt_matches takes it as it is.  warp_offset [B, 4, 2] displaces the corners (o, o), (o, H-o-1), (W-o-1, o),
    (W-o-1, H-o-1), in that order; None draws integers in [-offset, offset) on the device with torch.randint and `generator`."""
    B, H, W, C = _frames(frames, "frames")
    if isinstance(offset, bool) or not isinstance(offset, int) or offset < 0:
        raise ValueError(f"offset must be a non-negative int, got {offset!r}")
    if 2 * offset >= min(H, W):
        raise ValueError(f"2 * offset must be below min(H, W) = {min(H, W)}, got offset {offset}")
    if warp_offset is None:
        _lib.gpu_tensor(frames, "frames", torch.uint8)
        warp_offset = _draw(B, offset, frames.device, generator)
    else:
        _offsets(warp_offset, B)
    image0, image1, Ht = _pairs(frames, B, H, W, C, offset, warp_offset, None)
    return _item(image0, image1, Ht)


def warping_pairs(frames_grey, max_offset: int = 300, warp_offset=None, generator=None) -> Dict[str, Any]:
    """The MegaDepth-warping item for a batch.  frames_grey uint8 [B, H, W] (or [B, H, W, 1]) -> the dictionary of homography_pairs at full
    size; here H = transform(corners -> corners + warp_offset), corners (0, 0), (0, H-1), (W-1, 0), (W-1, H-1), is both the warp and
    the returned matrix (float32).  warp_offset None draws integers in [-max_offset, max_offset) (the reference: 300)."""
    B, H, W, _ = _frames(frames_grey, "frames_grey", channels=(1,))
    if isinstance(max_offset, bool) or not isinstance(max_offset, int) or max_offset < 0:
        raise ValueError(f"max_offset must be a non-negative int, got {max_offset!r}")
    if warp_offset is None:
        _lib.gpu_tensor(frames_grey, "frames_grey", torch.uint8)
        warp_offset = _draw(B, max_offset, frames_grey.device, generator)
    else:
        _offsets(warp_offset, B)
    wo = _lib.gpu_tensor(warp_offset, "warp_offset", convert=True)
    c = torch.tensor([[0, 0], [0, H - 1], [W - 1, 0], [W - 1, H - 1]], dtype=torch.float32, device=wo.device).expand(B, 4, 2)
    M = get_perspective_transform(c, c + wo)
    image0, image1, _ = _pairs(frames_grey, B, H, W, 1, 0, None, M)
    return _item(image0, image1, M.to(torch.float32))
