"""Numpy restatement of the homography training pairs (openglue_amd.pairs, csrc/pairs.hip): the specification the kernels are held to,
bit for bit.  Integer and float64 operations only (plus the final float32 division by 255); written from the arithmetic below, not
from any implementation.

  get_perspective_transform   point i: row i = [x y 1 0 0 0 -xu -yu | u], row i + 4 = [0 0 0 x y 1 -xv -yv | v]; np.linalg.solve in
                              float64, M[2][2] = 1.  A singular system (LinAlgError, a reciprocal condition number at the level of
                              rounding, or a non-finite solution) gives M = 0.
  get_perspective_transform_eliminated
                              the same system by the Gaussian elimination with partial pivoting that the kernel states, operation
                              for operation.  Two float64 solvers agree to about 1e-13 px on the corners but not in the last bit,
                              and the order of operations inside LAPACK varies with its build, so the items below, whose outputs
                              are compared bit for bit, take their matrices from this one.
  invert3                     Mi = adj(M) * (1 / det M), det along the first row; Mi = 0 when det == 0.
  source_xy                   destination pixel (x, y):  Wd = (Mi20 x + Mi21 y) + Mi22;  s = 32 / Wd (0 when Wd == 0);
                              fX = ((Mi00 x + Mi01 y) + Mi02) s, fY likewise; fX > INT_MAX -> INT_MAX, not fX >= INT_MIN -> INT_MIN;
                              X = rint(fX), Y = rint(fY): half to even.
  warp_perspective            sx = X >> 5, fx = X & 31 (same for y); taps (sy, sx), (sy, sx + 1), (sy + 1, sx), (sy + 1, sx + 1), 0 outside
                              the source; weights 32 (32 - fx)(32 - fy), 32 fx (32 - fy), 32 (32 - fx) fy, 32 fx fy;
                              out = (sum w v + 16384) >> 15 per channel.  Only the window (x0, y0, w, h) of the destination is formed.
  grey                        (9798 R + 19235 G + 3735 B + 16384) >> 15; one channel: the byte itself.
  homography_pairs            data/oxford_paris_dataset.py:32-66 without the colour augmentation, for a batch.
  warping_pairs               data/megadepth_dataset.py:41-52 for a batch (float32 division by 255).
"""
from __future__ import annotations

import numpy as np

INT_MAX, INT_MIN = 2147483647.0, -2147483648.0
SINGULAR_RCOND = 1e-12


def system(src, dst):
    """src, dst [4, 2] -> A [8, 8], b [8] float64"""
    src, dst = np.asarray(src, np.float64), np.asarray(dst, np.float64)
    A, b = np.zeros((8, 8)), np.zeros(8)
    for i in range(4):
        (x, y), (u, v) = src[i], dst[i]
        A[i] = [x, y, 1, 0, 0, 0, -x * u, -y * u]
        A[i + 4] = [0, 0, 0, x, y, 1, -x * v, -y * v]
        b[i], b[i + 4] = u, v
    return A, b


def get_perspective_transform(src, dst) -> np.ndarray:
    """src, dst [B, 4, 2] (or [4, 2]) -> M [B, 3, 3] (or [3, 3]) float64"""
    src, dst = np.asarray(src), np.asarray(dst)
    if src.ndim == 2:
        return get_perspective_transform(src[None], dst[None])[0]
    out = np.zeros((src.shape[0], 3, 3))
    for k in range(src.shape[0]):
        A, b = system(src[k], dst[k])
        try:
            if not 1.0 / np.linalg.cond(A) > SINGULAR_RCOND:
                continue
            x = np.linalg.solve(A, b)
        except np.linalg.LinAlgError:
            continue
        if np.all(np.isfinite(x)):
            out[k] = np.append(x, 1.0).reshape(3, 3)
    return out


def eliminate(A, b):
    """The 8 x 8 system by the elimination csrc/pairs.hip states, operation for operation in Python floats (IEEE float64, nothing
    fused): partial pivoting by the first largest |entry| of the column, a[i][j] -= (a[i][k] / a[k][k]) a[k][j], back substitution.
    None for a pivot not above 1e-12 max |coefficient| or a non-finite solution."""
    a = [[float(v) for v in row] + [float(r)] for row, r in zip(A, b)]
    tiny = SINGULAR_RCOND * max(abs(v) for row in a for v in row[:8])
    for k in range(8):
        p, best = k, abs(a[k][k])
        for i in range(k + 1, 8):
            if abs(a[i][k]) > best:
                p, best = i, abs(a[i][k])
        if not best > tiny:
            return None
        a[k], a[p] = a[p], a[k]
        for i in range(k + 1, 8):
            f = a[i][k] / a[k][k]
            for c in range(k + 1, 9):
                a[i][c] = a[i][c] - f * a[k][c]
    x = [0.0] * 8
    for i in range(7, -1, -1):
        s = a[i][8]
        for c in range(i + 1, 8):
            s = s - a[i][c] * x[c]
        x[i] = s / a[i][i]
        if not abs(x[i]) <= 1.7976931348623157e308:
            return None
    return x


def get_perspective_transform_eliminated(src, dst) -> np.ndarray:
    """get_perspective_transform with `eliminate` in place of np.linalg.solve: the kernels' solver to the bit.  LAPACK's own order of
    operations (blocked, fused multiply-adds, by build and machine) is not something a kernel can be bit-identical to; this is."""
    src, dst = np.asarray(src), np.asarray(dst)
    if src.ndim == 2:
        return get_perspective_transform_eliminated(src[None], dst[None])[0]
    out = np.zeros((src.shape[0], 3, 3))
    for k in range(src.shape[0]):
        x = eliminate(*system(src[k], dst[k]))
        if x is not None:
            out[k] = np.array(x + [1.0]).reshape(3, 3)
    return out


def invert3(M) -> np.ndarray:
    a, b, c, d, e, f, g, h, i = [np.float64(v) for v in np.asarray(M, np.float64).reshape(9)]
    c00, c01, c02 = e * i - f * h, f * g - d * i, d * h - e * g
    det = (a * c00 + b * c01) + c * c02
    idet = np.float64(1.0) / det if det != 0 else np.float64(0.0)
    return np.array([[c00 * idet, (c * h - b * i) * idet, (b * f - c * e) * idet],
                     [c01 * idet, (a * i - c * g) * idet, (c * d - a * f) * idet],
                     [c02 * idet, (b * g - a * h) * idet, (a * e - b * d) * idet]])


def source_xy(Mi, xs, ys):
    """xs, ys: float64 arrays of destination coordinates -> X, Y int64 (values of an int32): source coordinates in 1/32 px"""
    with np.errstate(all="ignore"):
        Wd = (Mi[2, 0] * xs + Mi[2, 1] * ys) + Mi[2, 2]
        s = np.where(Wd != 0, 32.0 / np.where(Wd != 0, Wd, 1.0), 0.0)
        out = []
        for r in (0, 1):
            f = ((Mi[r, 0] * xs + Mi[r, 1] * ys) + Mi[r, 2]) * s
            f = np.where(f > INT_MAX, INT_MAX, f)
            f = np.where(f >= INT_MIN, f, INT_MIN)
            out.append(np.rint(f).astype(np.int64))
    return out


def weights(fx, fy):
    return 32 * (32 - fx) * (32 - fy), 32 * fx * (32 - fy), 32 * (32 - fx) * fy, 32 * fx * fy


def warp_one(img, M, x0, y0, w, h) -> np.ndarray:
    """img [H, W, C] uint8 -> [h, w, C] uint8"""
    H, W, C = img.shape
    ys, xs = np.meshgrid(np.arange(y0, y0 + h, dtype=np.float64), np.arange(x0, x0 + w, dtype=np.float64), indexing="ij")
    X, Y = source_xy(invert3(M), xs, ys)
    sx, fx, sy, fy = X >> 5, X & 31, Y >> 5, Y & 31
    acc = np.zeros((h, w, C), np.int64)
    src = img.astype(np.int64)
    for wt, ty, tx in zip(weights(fx, fy), (sy, sy, sy + 1, sy + 1), (sx, sx + 1, sx, sx + 1)):
        inside = (ty >= 0) & (ty < H) & (tx >= 0) & (tx < W)
        v = src[np.where(inside, ty, 0), np.where(inside, tx, 0)]
        acc += np.where(inside, wt, 0)[..., None] * v
    return ((acc + 16384) >> 15).astype(np.uint8)


def warp_perspective(images, M, dsize=None, origin=(0, 0)) -> np.ndarray:
    """images [B, H, W, C] uint8, M [B, 3, 3] float64, dsize (w, h) -> [B, h, w, C] uint8"""
    B, H, W, C = images.shape
    w, h = (W, H) if dsize is None else dsize
    return np.stack([warp_one(images[b], M[b], origin[0], origin[1], w, h) for b in range(B)])


def grey(img) -> np.ndarray:
    """[..., C] uint8 -> [...] int64"""
    v = img.astype(np.int64)
    if img.shape[-1] == 1:
        return v[..., 0]
    return (9798 * v[..., 0] + 19235 * v[..., 1] + 3735 * v[..., 2] + 16384) >> 15


def to_unit(g) -> np.ndarray:
    return g.astype(np.float32) / np.float32(255.0)


def corners(H, W, offset) -> np.ndarray:
    o = offset
    return np.array([[o, o], [o, H - o - 1], [W - o - 1, o], [W - o - 1, H - o - 1]], dtype=np.float32)


def homography_pairs(frames, offset, warp_offset, solver=None):
    """frames [B, H, W, C] uint8, warp_offset [B, 4, 2] float32 -> image0, image1 [B, 1, h, w] float32, H_true [B, 3, 3] float32,
    H_warp [B, 3, 3] float64.  solver: get_perspective_transform_eliminated unless given"""
    solver = solver or get_perspective_transform_eliminated
    B, H, W, C = frames.shape
    wo = np.asarray(warp_offset, np.float32)
    full = corners(H, W, offset)[None].repeat(B, 0)
    crop = corners(H - 2 * offset, W - 2 * offset, 0)[None].repeat(B, 0)
    H_warp = solver(full + wo, full)                              # float32 sums, as the reference hands them to cv2
    H_true = solver(crop + wo, crop).astype(np.float32)
    w, h = W - 2 * offset, H - 2 * offset
    warped = warp_perspective(frames, H_warp, (w, h), (offset, offset))
    image0 = to_unit(grey(frames[:, offset:H - offset, offset:W - offset]))[:, None]
    image1 = to_unit(grey(warped))[:, None]
    return image0, image1, H_true, H_warp


def warping_pairs(frames, warp_offset, solver=None):
    """frames [B, H, W] uint8 -> image0, image1 [B, 1, H, W] float32, H [B, 3, 3] float32 (the warp matrix itself)"""
    B, H, W = frames.shape
    c = corners(H, W, 0)[None].repeat(B, 0)
    M = (solver or get_perspective_transform_eliminated)(c, c + np.asarray(warp_offset, np.float32))
    warped = warp_perspective(frames[..., None], M)
    return to_unit(frames.astype(np.int64))[:, None], to_unit(warped[..., 0].astype(np.int64))[:, None], M.astype(np.float32), M
