"""Numpy restatement of the MegaDepth training pairs (openglue_amd.megadepth, csrc/megadepth.hip): the specification the kernels are
held to, bit for bit.  Written from the arithmetic below and from what the reference's data items mean, not from any implementation.
The per-item functions go the reference's way -- grey, resize of the whole image, crop, then indexing -- so that the fused kernels,
which only ever form the crop window, are checked against the unfused meaning.

  linear_taps          destination index d of a `dst`-long axis resized from `src`: scale = 1.0 / (dst / src) in double;
                       f = float32((d + 0.5) scale - 0.5); s = floor(f); f -= s; s < 0 -> s = 0, f = 0; s >= src - 1 -> s = src - 1, f = 0;
                       the second tap is min(s + 1, src - 1) (its weight is 0 where it was clamped).
  resize_linear_u8     cv2.resize(..., INTER_LINEAR) on bytes: coefficients rint((1 - f) 2048), rint(f 2048) (half to even), horizontal pass
                       S[s] a0 + S[s + 1] a1 in int32, vertical (((b0 (R0 >> 4)) >> 16) + ((b1 (R1 >> 4)) >> 16) + 2) >> 2.
  resize_f32           'linear': the same taps, float32 coefficients 1 - f and f, S[s] a0 + S[s + 1] a1 then R0 b0 + R1 b1, every product and
                       sum rounded on its own; 'nearest': s = min(floor(d (1.0 / (dst / src))), src - 1) in double.
  grey                 (9798 R + 19235 G + 3735 B + 16384) >> 15; one channel: the byte itself.
  scale_K              diag(resize_w / w, resize_h / h, 1).astype(float32) @ K, then K[axis, 2] -= start.
  megadepth_item       data/megadepth_dataset.py:125-178 for one frame;  megadepth_pairs: the batch after the default collate.
  feature_item         data/megadepth_dataset.py:208-260 for one image;  stack_keypoints: data/megadepth_datamodule.py:137-164 for one image, with
                       the selection rule of openglue_amd.megadepth (the num_keypoints largest keys in descending order, the lower index first
                       on ties) and depth 0 where the reference would raise or wrap (an index outside the cropped map).
"""
from __future__ import annotations

import numpy as np


def linear_taps(src: int, dst: int):
    """-> s0, s1 [dst] int64, f [dst] float32"""
    scale = 1.0 / (dst / src)
    d = np.arange(dst, dtype=np.float64)
    f = ((d + 0.5) * scale - 0.5).astype(np.float32)
    fl = np.floor(f)
    s = fl.astype(np.int64)
    f = (f - fl).astype(np.float32)
    low, high = s < 0, s >= src - 1
    s = np.where(low, 0, np.where(high, src - 1, s))
    f = np.where(low | high, np.float32(0), f).astype(np.float32)
    return s, np.minimum(s + 1, src - 1), f


def nearest_index(src: int, dst: int) -> np.ndarray:
    d = np.arange(dst, dtype=np.float64)
    return np.minimum(np.floor(d * (1.0 / (dst / src))).astype(np.int64), src - 1)


def _window(full, dsize, origin, window):
    dw, dh = dsize
    x0, y0 = origin
    w, h = (dw - x0, dh - y0) if window is None else window
    assert 0 <= x0 and 0 <= y0 and w >= 1 and h >= 1 and x0 + w <= dw and y0 + h <= dh
    return full[:, y0:y0 + h, x0:x0 + w]


def resize_linear_u8(images, dsize, origin=(0, 0), window=None) -> np.ndarray:
    """images uint8 [B, H, W] or [B, H, W, C] -> the window (origin (x0, y0), size (w, h); default: up to the far corner) of the images
    resized to dsize = (dw, dh).  The whole resized image is formed and then cut."""
    images = np.asarray(images)
    assert images.dtype == np.uint8 and images.ndim in (3, 4)
    H, W = images.shape[1:3]
    dw, dh = dsize
    sx0, sx1, fx = linear_taps(W, dw)
    sy0, sy1, fy = linear_taps(H, dh)
    a1 = np.rint(fx * np.float32(2048)).astype(np.int64)
    a0 = np.rint((np.float32(1) - fx) * np.float32(2048)).astype(np.int64)
    b1 = np.rint(fy * np.float32(2048)).astype(np.int64)
    b0 = np.rint((np.float32(1) - fy) * np.float32(2048)).astype(np.int64)
    S = images.astype(np.int64)
    tail = (1,) * (images.ndim - 3)
    a0, a1 = a0.reshape((1, 1, dw) + tail), a1.reshape((1, 1, dw) + tail)
    b0, b1 = b0.reshape((1, dh, 1) + tail), b1.reshape((1, dh, 1) + tail)
    rows = S[:, :, sx0] * a0 + S[:, :, sx1] * a1                       # [B, H, dw(, C)]
    R0, R1 = rows[:, sy0], rows[:, sy1]
    out = (((b0 * (R0 >> 4)) >> 16) + ((b1 * (R1 >> 4)) >> 16) + 2) >> 2
    assert out.min() >= 0 and out.max() <= 255
    return _window(out.astype(np.uint8), dsize, origin, window)


def resize_f32(maps, dsize, interpolation="linear", origin=(0, 0), window=None) -> np.ndarray:
    """maps float32 [B, H, W] -> the window of the maps resized to dsize = (dw, dh)"""
    maps = np.asarray(maps)
    assert maps.dtype == np.float32 and maps.ndim == 3
    H, W = maps.shape[1:]
    dw, dh = dsize
    if interpolation == "nearest":
        out = maps[:, nearest_index(H, dh)][:, :, nearest_index(W, dw)]
    elif interpolation == "linear":
        sx0, sx1, fx = linear_taps(W, dw)
        sy0, sy1, fy = linear_taps(H, dh)
        one = np.float32(1)
        with np.errstate(all="ignore"):
            rows = (maps[:, :, sx0] * (one - fx) + maps[:, :, sx1] * fx).astype(np.float32)
            out = (rows[:, sy0] * (one - fy)[None, :, None] + rows[:, sy1] * fy[None, :, None]).astype(np.float32)
    else:
        raise ValueError(interpolation)
    return _window(out, dsize, origin, window)


def grey(frames) -> np.ndarray:
    """uint8 [..., H, W, 3] (RGB) or [..., H, W] -> uint8 [..., H, W]"""
    frames = np.asarray(frames)
    if frames.ndim >= 3 and frames.shape[-1] == 3:
        v = frames.astype(np.int64)
        return ((9798 * v[..., 0] + 19235 * v[..., 1] + 3735 * v[..., 2] + 16384) >> 15).astype(np.uint8)
    if frames.ndim >= 3 and frames.shape[-1] == 1:
        return frames[..., 0]
    return frames


def to_unit(g) -> np.ndarray:
    return np.asarray(g).astype(np.float32) / np.float32(255)


def scale_K(K, size, resized, axis, start) -> np.ndarray:
    """size (w, h) -> resized (resize_w, resize_h): the reference's np.dot(scales, K), then the crop's shift"""
    scales = np.diag([resized[0] / size[0], resized[1] / size[1], 1.0]).astype(np.float32)
    K = np.dot(scales, np.asarray(K, np.float32))
    if axis in (0, 1):
        K[axis, 2] -= start
    assert K.dtype == np.float32
    return K


def megadepth_item(frame, depth, K, target_size, plan, depth_interpolation="linear"):
    """One frame of MegaDepthPairsDataset.__getitem__: frame uint8 [H, W, 3] or [H, W], depth float32 [H, W], plan = (resize_w, resize_h, axis,
    start) from crop_plan -> image float32 [th, tw] in [0, 1], depth float32 [th, tw], K float32 [3, 3]"""
    tw, th = target_size
    rw, rh, axis, start = plan
    g = grey(frame)
    H, W = g.shape
    image = resize_linear_u8(g[None], (rw, rh))[0]
    d = resize_f32(np.asarray(depth, np.float32)[None], (rw, rh), depth_interpolation)[0]
    if axis == 0:
        image, d = image[:, start:start + tw], d[:, start:start + tw]
    else:
        image, d = image[start:start + th, :], d[start:start + th, :]
    assert image.shape == (th, tw) and d.shape == (th, tw)
    return to_unit(image), d, scale_K(K, (W, H), (rw, rh), axis, start)


def megadepth_pairs(frames0, frames1, depth0, depth1, K0, K1, target_size, plans0, plans1, depth_interpolation="linear"):
    """-> image0, image1 [B, 1, th, tw], depth0, depth1 [B, th, tw], K0, K1 [B, 3, 3], all float32"""
    out = []
    for frames, depths, Ks, plans in ((frames0, depth0, K0, plans0), (frames1, depth1, K1, plans1)):
        items = [megadepth_item(f, d, K, target_size, p, depth_interpolation) for f, d, K, p in zip(frames, depths, Ks, plans)]
        out.append([np.stack([it[k] for it in items]) for k in range(3)])
    (i0, d0, k0), (i1, d1, k1) = out
    return i0[:, None], i1[:, None], d0, d1, k0, k1


def feature_item(lafs, scores, descriptors, image_size, orig_size, depth, K, target_size, plan):
    """One image of MegaDepthPairsDatasetFeatures.__getitem__: plan = (axis, start) from feature_crop_plan (axis -1: no crop) ->
    lafs, scores, descriptors of the keypoints inside the crop (shifted), the cropped nearest-resized depth map, K"""
    tw, th = target_size
    axis, start = plan
    lafs, scores, descriptors = np.array(lafs, np.float32), np.asarray(scores, np.float32), np.asarray(descriptors, np.float32)
    d = resize_f32(np.asarray(depth, np.float32)[None], tuple(image_size), "nearest")[0]
    K = scale_K(K, orig_size, image_size, axis, start)
    if axis in (0, 1):
        end = start + (tw, th)[axis]
        d = d[:, start:end] if axis == 0 else d[start:end, :]
        mask = (lafs[:, axis, 2] >= start) & (lafs[:, axis, 2] < end)
        lafs = lafs[mask]
        lafs[:, axis, 2] -= start
        scores, descriptors = scores[mask], descriptors[mask]
    assert lafs.dtype == np.float32
    return lafs, scores, descriptors, d, K


def select(keys, k) -> np.ndarray:
    """indices of the k largest keys, descending, the lower index first on ties"""
    return np.argsort(-np.asarray(keys, np.float64), kind="stable")[:k]


def stack_keypoints(lafs, scores, descriptors, depth_map, num_keypoints, keys=None):
    """One image of stack_keypoints_batch: -> lafs [k, 2, 3], scores [k], descriptors [k, D], depth [k], zero padded.  keys: what the
    selection ranks when more than k keypoints are there (None: the scores)."""
    n, D = lafs.shape[0], descriptors.shape[1]
    L, S = np.zeros((num_keypoints, 2, 3), np.float32), np.zeros(num_keypoints, np.float32)
    Dm, dp = np.zeros((num_keypoints, D), np.float32), np.zeros(num_keypoints, np.float32)
    idx = select(scores if keys is None else keys, num_keypoints) if n > num_keypoints else np.arange(n)
    m = len(idx)
    L[:m], S[:m], Dm[:m] = lafs[idx], scores[idx], descriptors[idx]
    x, y = L[:m, 0, 2].astype(np.int64), L[:m, 1, 2].astype(np.int64)          # truncation, as Tensor.type(torch.int64)
    inside = (L[:m, 0, 2] > -1) & (L[:m, 1, 2] > -1) & (x < depth_map.shape[1]) & (y < depth_map.shape[0])
    dp[:m] = np.where(inside, depth_map[np.where(inside, y, 0), np.where(inside, x, 0)], np.float32(0)) if depth_map.size else 0
    return L, S, Dm, dp


def feature_pairs_side(items, target_size, num_keypoints, plans, keys=None):
    """items: per image (lafs, scores, descriptors, image_size, orig_size, depth, K) -> lafs [B, k, 2, 3], scores [B, k], descriptors [B, k, D],
    depth [B, k], K [B, 3, 3]; keys: per image, over ALL its keypoints (before the crop), or None"""
    out = []
    for i, (it, plan) in enumerate(zip(items, plans)):
        lafs, scores, desc, image_size, orig_size, depth, K = it
        l, s, d, dm, Kc = feature_item(lafs, scores, desc, image_size, orig_size, depth, K, target_size, plan)
        kk = None
        if keys is not None:
            kk = np.asarray(keys[i], np.float32)
            if plan[0] in (0, 1):
                c = np.asarray(lafs, np.float32)[:, plan[0], 2]
                kk = kk[(c >= plan[1]) & (c < plan[1] + target_size[plan[0]])]
        out.append(stack_keypoints(l, s, d, dm, num_keypoints, kk) + (Kc,))
    return tuple(np.stack([o[j] for o in out]) for j in range(5))
