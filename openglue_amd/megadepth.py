"""MegaDepth training pairs on HIP kernels: the main stage of the reference's recipe (train.py with config/config.yaml, train_cached.py with
config_cached.yaml), whose samples the reference prepares with cv2 and numpy in its data-loader workers (data/megadepth_dataset.py:119-192
MegaDepthPairsDataset.__getitem__, :203-282 MegaDepthPairsDatasetFeatures.__getitem__, data/megadepth_datamodule.py:105-166
stack_keypoints_batch).  Here a batch of decoded frames of differing sizes, their depth maps and intrinsics become the training item
without leaving the GPU; the loader only decodes.

  crop_plan, feature_crop_plan   the reference's resize and crop arithmetic, plain Python on the host
  resize_linear_u8               cv2.resize(INTER_LINEAR) on uint8, restricted to a destination window (also what extract_features.read_image needs)
  resize_f32                     the same for float maps, 'linear' or 'nearest'
  megadepth_pairs                the online item for a whole batch: {'image0', 'image1', 'transformation'} as after the default collate
  megadepth_feature_pairs        the cached item and its collate for a whole batch

Thin wrappers over og_resize_linear_u8 / og_resize_f32 / og_megadepth_pairs / og_megadepth_features (include/openglue_amd.h,
csrc/megadepth.hip); GPU tensors only, no host synchronisation: the per-image geometry travels in a small table that is copied to the
device without blocking.  The kernels are bit-identical to the numpy restatement in tests/megadepth_ref.py, from run to run and whatever
the batch.  cv2 itself was not available to compare with; DESIGN.md 4.15 lists where its builds may differ.

Out of scope: decoding (JPEG, HDF5 depth), the pairs list, and extracting the cached features.
"""
from __future__ import annotations

import ctypes
from typing import Any, Dict, List, Optional, Sequence, Tuple

import torch

from . import _lib
from .geometry import _shape
from .pairs import _frames

MAX_FRAMES, MAX_SIDE, MAX_KEYPOINTS, MAX_SELECTED = 65535, 32768, 8192, 4096


def _pair(v, name: str) -> Tuple[int, int]:
    try:
        a, b = v
    except (TypeError, ValueError):
        raise ValueError(f"{name} must be two integers (width, height), got {v!r}") from None
    for x in (a, b):
        if isinstance(x, bool) or int(x) != x:
            raise ValueError(f"{name} must be two integers (width, height), got {v!r}")
    return int(a), int(b)


def _start(start, room: int, low_inclusive_high: int, random_crop: bool, generator) -> int:
    """the crop's start: given (0 <= start <= room), drawn in [0, low_inclusive_high) on the CPU, or centred"""
    if start is not None:
        if isinstance(start, bool) or int(start) != start or not 0 <= start <= room:
            raise ValueError(f"start must be an integer in [0, {room}], got {start!r}")
        return int(start)
    if random_crop:
        return int(torch.randint(0, low_inclusive_high, (1,), generator=generator).item())
    return room // 2


def crop_plan(size, target_size, random_crop: bool = False, start: Optional[int] = None, generator=None) -> Tuple[int, int, int, int]:
    """MegaDepthPairsDataset's plan for an image of `size` (w, h) and `target_size` (tw, th) -> (resize_w, resize_h, axis, start): resize to
    resize_w x resize_h, then cut [start, start + target) along axis 0 (width) or 1 (height).  The reference's arithmetic in Python floats as
    it is written there; the start is (resized - target) // 2, or with random_crop an integer in [0, max(resized - target, 1)) drawn on the CPU
    with torch.randint and `generator` (a CPU generator), or `start` as given.  ValueError if a resized side would fall below the target,
    where the reference would silently return an empty image."""
    w, h = _pair(size, "size")
    tw, th = _pair(target_size, "target_size")
    if min(w, h, tw, th) < 1:
        raise ValueError(f"size {size!r} and target_size {target_size!r} must be positive")
    current_ratio = w / h
    target_ratio = tw / th
    if current_ratio > target_ratio:
        resize_h = th
        resize_w = int(current_ratio * resize_h)
        axis, room = 0, resize_w - tw
    else:
        resize_w = tw
        resize_h = int(resize_w / current_ratio)
        axis, room = 1, resize_h - th
    if room < 0:
        raise ValueError(f"a {w} x {h} image resized to {resize_w} x {resize_h} falls below the target {tw} x {th}")
    return resize_w, resize_h, axis, _start(start, room, max(room, 1), random_crop, generator)


def feature_crop_plan(image_size, target_size, random_crop: bool = False, start: Optional[int] = None, generator=None) -> Tuple[int, int]:
    """MegaDepthPairsDatasetFeatures' rule for features extracted at `image_size` (w, h) -> (axis, start): crop the width if tw < w, else the
    height if th < h, else nothing (axis -1, start 0).  Centre start (image - target) // 2, or with random_crop an integer in
    [0, image - target) drawn on the CPU with torch.randint and `generator`, or `start` as given."""
    w, h = _pair(image_size, "image_size")
    tw, th = _pair(target_size, "target_size")
    if min(w, h, tw, th) < 1:
        raise ValueError(f"image_size {image_size!r} and target_size {target_size!r} must be positive")
    if tw < w:
        return 0, _start(start, w - tw, w - tw, random_crop, generator)
    if th < h:
        return 1, _start(start, h - th, h - th, random_crop, generator)
    if start not in (None, 0):
        raise ValueError(f"nothing to crop from {w} x {h} at the target {tw} x {th}: start must be 0, got {start!r}")
    return -1, 0


# ---------------------------------------------------------------- resize primitives
def _window(dsize, origin, window) -> Tuple[int, int, int, int, int, int]:
    dw, dh = _pair(dsize, "dsize")
    x0, y0 = _pair(origin, "origin")
    w, h = (dw - x0, dh - y0) if window is None else _pair(window, "window")
    if not (0 < dw <= MAX_SIDE and 0 < dh <= MAX_SIDE):
        raise ValueError(f"dsize must lie in [1, {MAX_SIDE}], got {dw} x {dh}")
    if w < 1 or h < 1 or x0 < 0 or y0 < 0 or x0 + w > dw or y0 + h > dh:
        raise ValueError(f"the window origin ({x0}, {y0}) size {w} x {h} must lie inside the resized {dw} x {dh} image")
    return dw, dh, x0, y0, w, h


def resize_linear_u8(images, dsize: Tuple[int, int], origin: Tuple[int, int] = (0, 0), window: Optional[Tuple[int, int]] = None) -> torch.Tensor:
    """cv2.resize(images[b], dsize) with the default INTER_LINEAR on bytes (11-bit integer coefficients), of which only the window with
    `origin` (x0, y0) and size `window` (w, h) (cv2's order; default: up to the far corner) is computed.  images uint8 [B, H, W],
    [B, H, W, 1] or [B, H, W, 3] -> uint8 [B, h, w] or [B, h, w, C]."""
    B, H, W, C = _frames(images, "images")
    dw, dh, x0, y0, w, h = _window(dsize, origin, window)
    src = _lib.gpu_tensor(images, "images", torch.uint8)
    out = torch.empty((B, h, w) if images.dim() == 3 else (B, h, w, C), device=src.device, dtype=torch.uint8)
    _lib.call("og_resize_linear_u8", src.device, B, H, W, C, src.data_ptr(), dw, dh, x0, y0, w, h, out.data_ptr(), _lib.STREAM)
    return out


_INTERPOLATIONS = {"linear": 0, "nearest": 1}


def _interpolation(name) -> int:
    if name not in _INTERPOLATIONS:
        raise ValueError(f"interpolation must be 'linear' or 'nearest', got {name!r}")
    return _INTERPOLATIONS[name]


def resize_f32(maps, dsize: Tuple[int, int], interpolation: str = "linear", origin: Tuple[int, int] = (0, 0),
               window: Optional[Tuple[int, int]] = None) -> torch.Tensor:
    """cv2.resize of float32 maps [B, H, W] -> [B, h, w]: 'linear' (INTER_LINEAR; float coefficients, every product and sum rounded on its
    own) or 'nearest' (INTER_NEAREST), restricted to a window as resize_linear_u8."""
    s = _shape(maps, "maps")
    mode = _interpolation(interpolation)
    if maps.dtype != torch.float32:
        raise ValueError(f"maps must be float32, got {maps.dtype}")
    if len(s) != 3 or not (0 < s[0] <= MAX_FRAMES and 0 < s[1] <= MAX_SIDE and 0 < s[2] <= MAX_SIDE):
        raise ValueError(f"maps must be [B, H, W] with 0 < B <= {MAX_FRAMES} and 0 < H, W <= {MAX_SIDE}, got {list(s)}")
    B, H, W = s
    dw, dh, x0, y0, w, h = _window(dsize, origin, window)
    src = _lib.gpu_tensor(maps, "maps")
    out = torch.empty(B, h, w, device=src.device, dtype=torch.float32)
    _lib.call("og_resize_f32", src.device, B, H, W, src.data_ptr(), dw, dh, mode, x0, y0, w, h, out.data_ptr(), _lib.STREAM)
    return out


# ---------------------------------------------------------------- the online item
def _table_to_device(table, dev: torch.device) -> torch.Tensor:
    """a ctypes array of table entries -> its bytes on the device, through pinned memory and without blocking the host"""
    host = torch.frombuffer(table, dtype=torch.uint8).pin_memory()
    return host.to(dev, non_blocking=True)


def _frame_list(frames, depths, side: int) -> List[Tuple[int, int, int]]:
    """(H, W, C) per frame, checked against its depth map; no device is touched"""
    out = []
    for i, (f, d) in enumerate(zip(frames, depths)):
        name = f"frames{side}[{i}]"
        s = _shape(f, name)
        if f.dtype != torch.uint8:
            raise ValueError(f"{name} must be uint8, got {f.dtype}")
        if len(s) == 2:
            s = s + (1,)
        if len(s) != 3 or s[2] not in (1, 3) or not (0 < s[0] <= MAX_SIDE and 0 < s[1] <= MAX_SIDE):
            raise ValueError(f"{name} must be [H, W] or [H, W, C] with C in {{1, 3}} and 0 < H, W <= {MAX_SIDE}, got {list(f.shape)}")
        if not isinstance(d, torch.Tensor) or d.dtype != torch.float32 or tuple(d.shape) != s[:2]:
            raise ValueError(f"depth{side}[{i}] must be a float32 tensor of its frame's size {list(s[:2])}")
        out.append(s)
    return out


def _batch_matrix(t, name: str, shape) -> None:
    if _shape(t, name) != shape:
        raise ValueError(f"{name} must be {list(shape)}, got {list(t.shape)}")


def megadepth_pairs(frames0: Sequence[torch.Tensor], frames1: Sequence[torch.Tensor], depth0: Sequence[torch.Tensor],
                    depth1: Sequence[torch.Tensor], K0, K1, R, T, target_size: Tuple[int, int], random_crop: bool = False, starts=None,
                    generator=None, depth_interpolation: str = "linear") -> Dict[str, Any]:
    """The MegaDepthPairsDataset item for a batch.  frames0, frames1: lists of B uint8 GPU tensors [H, W, 3] (RGB) or [H, W] whose sizes may all
    differ; depth0, depth1: float32 [H, W] of their frames' sizes; K0, K1, R [B, 3, 3], T [B, 3]; target_size (tw, th) ->
    {'image0', 'image1': float32 [B, 1, th, tw] in [0, 1], 'transformation': {'type': ['3d_reprojection'] * B, 'K0', 'K1', 'R', 'T',
    'depth0', 'depth1': float32 [B, th, tw]}}: what supervision.generate_gt_matches and metrics take as it is.  Every frame goes through
    crop_plan: centre crop, or random_crop with the CPU `generator`, or starts = (starts0, starts1), two lists of B integers.
    depth_interpolation: 'linear' is what the reference's call computes (its cv2.resize(depth, size, cv2.INTER_NEAREST) passes the constant as
    the `dst` argument, so the default interpolation applies); 'nearest' is what it appears to intend.  One table copy and two launches."""
    mode = _interpolation(depth_interpolation)
    tw, th = _pair(target_size, "target_size")
    B = len(frames0)
    if not (0 < 2 * B <= MAX_FRAMES) or any(len(v) != B for v in (frames1, depth0, depth1)):
        raise ValueError(f"frames0, frames1, depth0 and depth1 must be lists of the same length B with 0 < 2 B <= {MAX_FRAMES}")
    shapes = _frame_list(frames0, depth0, 0) + _frame_list(frames1, depth1, 1)
    for t, name, shape in ((K0, "K0", (B, 3, 3)), (K1, "K1", (B, 3, 3)), (R, "R", (B, 3, 3)), (T, "T", (B, 3))):
        _batch_matrix(t, name, shape)
    if starts is not None and (len(starts) != 2 or any(len(s) != B for s in starts)):
        raise ValueError("starts must be (starts0, starts1), two lists of B integers")
    given = [None] * (2 * B) if starts is None else list(starts[0]) + list(starts[1])
    plans = [crop_plan((W, H), (tw, th), random_crop, given[i], generator) for i, (H, W, _) in enumerate(shapes)]
    # everything below needs the GPU
    Kin = [_lib.gpu_tensor(K0, "K0", convert=True), _lib.gpu_tensor(K1, "K1", convert=True)]
    dev = Kin[0].device
    imgs = [_lib.gpu_tensor(f, "frames", torch.uint8) for f in list(frames0) + list(frames1)]
    deps = [_lib.gpu_tensor(d, "depth") for d in list(depth0) + list(depth1)]
    table = (_lib.og_md_frame * (2 * B))()
    for i, ((H, W, C), (rw, rh, axis, start)) in enumerate(zip(shapes, plans)):
        e = table[i]
        e.image, e.depth, e.K = imgs[i].data_ptr(), deps[i].data_ptr(), Kin[i // B].data_ptr() + 36 * (i % B)
        e.H, e.W, e.C, e.resize_w, e.resize_h = H, W, C, rw, rh
        e.x0, e.y0 = (start, 0) if axis == 0 else (0, start)
    images = torch.empty(2, B, 1, th, tw, device=dev, dtype=torch.float32)
    depths = torch.empty(2, B, th, tw, device=dev, dtype=torch.float32)
    Kout = torch.empty(2, B, 3, 3, device=dev, dtype=torch.float32)
    with torch.cuda.device(dev):
        table_dev = _table_to_device(table, dev)
    _lib.call("og_megadepth_pairs", dev, 2 * B, tw, th, ctypes.addressof(table), table_dev.data_ptr(), images.data_ptr(), depths.data_ptr(),
              Kout.data_ptr(), mode, _lib.STREAM)
    transformation = {"type": ["3d_reprojection"] * B, "K0": Kout[0], "K1": Kout[1], "R": _lib.gpu_tensor(R, "R", convert=True),
                      "T": _lib.gpu_tensor(T, "T", convert=True), "depth0": depths[0], "depth1": depths[1]}
    return {"image0": images[0], "image1": images[1], "transformation": transformation}


# ---------------------------------------------------------------- the cached item and its collate
def megadepth_feature_pairs(features0: Sequence[Dict[str, Any]], features1: Sequence[Dict[str, Any]], R, T, target_size: Tuple[int, int],
                            num_keypoints: int, random_crop: bool = False, starts=None, random: bool = False, generator=None,
                            keys=None) -> Dict[str, Any]:
    """MegaDepthPairsDatasetFeatures.__getitem__ followed by stack_keypoints_batch, for a batch.  features0, features1: lists of B dictionaries,
    one per image, with GPU tensors 'lafs' [N, 2, 3], 'scores' [N], 'descriptors' [N, D] (float32; N differs from image to image, 0 allowed),
    'depth' float32 [h, w] (the depth map at its original size), 'K' [3, 3], and 'image_size', 'orig_size' (w, h): the size the features were
    extracted at and the original image's.  R [B, 3, 3], T [B, 3] -> {'lafs0', 'lafs1' [B, k, 2, 3], 'scores0', 'scores1' [B, k],
    'descriptors0', 'descriptors1' [B, k, D], 'image0_size', 'image1_size': target_size, 'transformation': {'type': ['3d_reprojection'],
    'K0', 'K1', 'R', 'T', 'depth0', 'depth1' [B, k]}} with k = num_keypoints, zero padded (depth 0: supervision ignores the keypoint).

    Crop: feature_crop_plan per image (centre, random_crop with the CPU `generator`, or starts = (starts0, starts1)); keypoints outside are
    dropped, the others shifted.  At most k left: kept in their order.  More: the k largest keys are kept, in descending order, the lower
    index first on ties.  The key is the score, or with random=True one uniform draw per keypoint (torch.rand on the device with `generator`,
    a device generator then, used for the keys only): that gives every k-subset the same probability, as the reference's randperm(n)[:k]
    does, in another order -- the order of the keypoints has no meaning.  keys = (keys0, keys1), lists of [N] tensors, overrides both.
    Depth per keypoint is read from the original map through cv2's nearest-neighbour index map; the resized map is never built.  Unlike the
    reference, a keypoint whose truncated position falls outside the cropped image gets depth 0 (there: IndexError, or a wrapped index).
    One table copy and one launch for both sides."""
    tw, th = _pair(target_size, "target_size")
    B = len(features0)
    if not (0 < 2 * B <= MAX_FRAMES) or len(features1) != B:
        raise ValueError(f"features0 and features1 must be lists of the same length B with 0 < 2 B <= {MAX_FRAMES}")
    if isinstance(num_keypoints, bool) or not isinstance(num_keypoints, int) or not 0 < num_keypoints <= MAX_SELECTED:
        raise ValueError(f"num_keypoints must be an int in [1, {MAX_SELECTED}], got {num_keypoints!r}")
    _batch_matrix(R, "R", (B, 3, 3))
    _batch_matrix(T, "T", (B, 3))
    if starts is not None and (len(starts) != 2 or any(len(s) != B for s in starts)):
        raise ValueError("starts must be (starts0, starts1), two lists of B integers")
    if keys is not None and (len(keys) != 2 or any(len(s) != B for s in keys)):
        raise ValueError("keys must be (keys0, keys1), two lists of B tensors")
    given = [None] * (2 * B) if starts is None else list(starts[0]) + list(starts[1])
    items = list(features0) + list(features1)
    D = None
    geo = []
    for i, it in enumerate(items):
        name = f"features{i // B}[{i % B}]"
        n = _shape(it["scores"], f"{name}['scores']")
        if len(n) != 1 or n[0] > MAX_KEYPOINTS:
            raise ValueError(f"{name}['scores'] must be [N] with N <= {MAX_KEYPOINTS}, got {list(n)}")
        n = n[0]
        d = _shape(it["descriptors"], f"{name}['descriptors']")
        if _shape(it["lafs"], f"{name}['lafs']") != (n, 2, 3) or len(d) != 2 or d[0] != n or d[1] < 1 or (D is not None and d[1] != D):
            raise ValueError(f"{name}: lafs must be [N, 2, 3] and descriptors [N, D] with N = {n} and one D for the batch")
        D = d[1]
        dm = _shape(it["depth"], f"{name}['depth']")
        if len(dm) != 2 or not (0 < dm[0] <= MAX_SIDE and 0 < dm[1] <= MAX_SIDE) or _shape(it["K"], f"{name}['K']") != (3, 3):
            raise ValueError(f"{name}: depth must be [h, w] with 0 < h, w <= {MAX_SIDE} and K [3, 3]")
        iw, ih = _pair(it["image_size"], f"{name}['image_size']")
        ow, oh = _pair(it["orig_size"], f"{name}['orig_size']")
        if not all(0 < v <= MAX_SIDE for v in (iw, ih, ow, oh)):
            raise ValueError(f"{name}: image_size and orig_size must lie in [1, {MAX_SIDE}]")
        geo.append((n, iw, ih, ow, oh, dm[1], dm[0]) + feature_crop_plan((iw, ih), (tw, th), random_crop, given[i], generator))
    # everything below needs the GPU
    Rd, Td = _lib.gpu_tensor(R, "R", convert=True), _lib.gpu_tensor(T, "T", convert=True)
    dev = Rd.device
    f32 = lambda t, name: _lib.gpu_tensor(t, name, convert=True)
    held = [[f32(it[k], k) for k in ("lafs", "scores", "descriptors", "depth", "K")] for it in items]
    if keys is not None:
        ks = [f32(t, "keys") for t in list(keys[0]) + list(keys[1])]
        if any(tuple(t.shape) != (g[0],) for t, g in zip(ks, geo)):
            raise ValueError("every keys tensor must be [N] of its image")
    elif random:
        drawn = torch.rand(max(sum(g[0] for g in geo), 1), device=dev, generator=generator)
        ks, at = [], 0
        for g in geo:
            ks.append(drawn[at:at + g[0]])
            at += g[0]
    else:
        ks = [None] * (2 * B)
    table = (_lib.og_md_features * (2 * B))()
    for e, (lafs, scores, desc, depth, K), key, g in zip(table, held, ks, geo):
        e.lafs, e.scores, e.descriptors, e.depth, e.K = (t.data_ptr() or None for t in (lafs, scores, desc, depth, K))
        e.keys = None if key is None or g[0] == 0 else key.data_ptr()
        e.n, e.image_w, e.image_h, e.orig_w, e.orig_h, e.depth_w, e.depth_h, e.axis, e.start = g
    k = num_keypoints
    lafs = torch.empty(2, B, k, 2, 3, device=dev, dtype=torch.float32)
    scores = torch.empty(2, B, k, device=dev, dtype=torch.float32)
    desc = torch.empty(2, B, k, D, device=dev, dtype=torch.float32)
    depth = torch.empty(2, B, k, device=dev, dtype=torch.float32)
    Kout = torch.empty(2, B, 3, 3, device=dev, dtype=torch.float32)
    with torch.cuda.device(dev):
        table_dev = _table_to_device(table, dev)
    _lib.call("og_megadepth_features", dev, 2 * B, tw, th, k, D, ctypes.addressof(table), table_dev.data_ptr(), lafs.data_ptr(), scores.data_ptr(),
              desc.data_ptr(), depth.data_ptr(), Kout.data_ptr(), _lib.STREAM)
    transformation = {"type": ["3d_reprojection"], "K0": Kout[0], "K1": Kout[1], "R": Rd, "T": Td, "depth0": depth[0], "depth1": depth[1]}
    return {"lafs0": lafs[0], "scores0": scores[0], "descriptors0": desc[0], "lafs1": lafs[1], "scores1": scores[1], "descriptors1": desc[1],
            "image0_size": (tw, th), "image1_size": (tw, th), "transformation": transformation}
