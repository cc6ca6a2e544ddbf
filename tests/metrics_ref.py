"""Float64 restatement of the reference's utils/metrics.py formulas (and the kornia 0.6 functions it calls), for the tests of
openglue_amd.metrics.  Torch ops on CPU tensors, one pair at a time unless a function says otherwise."""
import math

import torch


def essential_from_Rt(R, T):
    """kornia essential_from_Rt(R1=I, t1=0, R2=R, t2=T) = [T]x R."""
    R, T = R.double(), T.double().reshape(3)
    tx = torch.zeros(3, 3, dtype=torch.float64)
    tx[0, 1], tx[0, 2], tx[1, 0], tx[1, 2], tx[2, 0], tx[2, 1] = -T[2], T[1], T[2], -T[0], -T[1], T[0]
    return tx @ R


def normalize_with_intrinsics(kpts, K):
    """utils/misc.py:5-7: (x - c) / f."""
    kpts, K = kpts.double(), K.double()
    return (kpts - K[:2, 2].unsqueeze(0)) / K[[0, 1], [0, 1]].unsqueeze(0)


def symmetrical_epipolar_distance(x0, x1, E):
    """kornia 0.6 symmetrical_epipolar_distance, squared=True: (x1^T E x0)^2 (1/|(E x0)_01|^2 + 1/|(E^T x1)_01|^2)."""
    h0 = torch.cat([x0, torch.ones_like(x0[:, :1])], 1)
    h1 = torch.cat([x1, torch.ones_like(x1[:, :1])], 1)
    l1 = h0 @ E.T                  # E x0, lines in image 1
    l0 = h1 @ E                    # E^T x1, lines in image 0
    num = (h1 * l1).sum(1) ** 2
    return num * (1.0 / (l1[:, :2] ** 2).sum(1) + 1.0 / (l0[:, :2] ** 2).sum(1))


def epipolar_distances(kpts0, kpts1, matches0, K0, K1, R, T, num_keypoints0=None):
    """One pair in the SuperGlue.match layout -> (distances of the matched keypoints in index order, matched mask [M])."""
    M = kpts0.shape[0]
    lim = M if num_keypoints0 is None else min(int(num_keypoints0), M)
    m = matches0.long()
    mask = (m >= 0) & (m < kpts1.shape[0]) & (torch.arange(M) < lim)
    x0 = normalize_with_intrinsics(kpts0[mask], K0)
    x1 = normalize_with_intrinsics(kpts1[m[mask]], K1)
    return symmetrical_epipolar_distance(x0, x1, essential_from_Rt(R, T)), mask


def precision_counts(dist, num_detected, threshold):
    """utils/metrics.py:37-44 -> (num_correct, precision, matching_score)."""
    n = int(dist.numel())
    if n == 0:
        return 0, 0.0, 0.0
    c = int((dist < threshold).sum())
    return c, c / n, c / num_detected


def rotation_error(R_true, R_pred):
    """degrees; utils/metrics.py:66-68."""
    c = ((R_true.double() * R_pred.double()).sum() - 1) / 2
    return abs(math.degrees(math.acos(max(-1.0, min(1.0, float(c))))))


def translation_error(T_true, T_pred):
    """degrees, min(a, 180 - a); utils/metrics.py:70-74, the cosine clamped to [-1, 1]."""
    a, b = T_true.double().reshape(3), T_pred.double().reshape(3)
    c = float(a @ b / max(float(a.norm() * b.norm()), 1e-8))
    ang = abs(math.degrees(math.acos(max(-1.0, min(1.0, c)))))
    return min(ang, 180.0 - ang)


def pose_error(R_true, T_true, R_pred, T_pred):
    return max(rotation_error(R_true, R_pred), translation_error(T_true, T_pred))


def ransac_threshold(thr_px, K0, K1):
    """utils/metrics.py:90, in fp32 as the reference computes it: 2 thr / mean(K0[0,0] + K1[0,0], K0[1,1] + K1[1,1])."""
    K0, K1 = K0.float(), K1.float()
    return float(2 * thr_px / (K0[[0, 1], [0, 1]] + K1[[0, 1], [0, 1]]).mean())


def sampson_error(x0, x1, E):
    """squared Sampson error of calibrated correspondences [n, 2] under E (x1^T E x0 = 0), fp64."""
    h0 = torch.cat([x0, torch.ones_like(x0[:, :1])], 1).double()
    h1 = torch.cat([x1, torch.ones_like(x1[:, :1])], 1).double()
    a = h0 @ E.double().T
    b = h1 @ E.double()
    num = (h1 * a).sum(1)
    return num ** 2 / (a[:, 0] ** 2 + a[:, 1] ** 2 + b[:, 0] ** 2 + b[:, 1] ** 2)


def pose_auc(errors, thresholds):
    """utils/metrics.py:125-141 in plain Python (fp64): -> {f'AUC@{t}deg': area}.  Keys follow the reference's f-string of a
    0-d tensor, i.e. of float(t) for float thresholds."""
    e = sorted(float(v) for v in errors)
    n = len(e)
    errs = [0.0] + e
    rec = [0.0] + [(i + 1) / n for i in range(n)]
    out = {}
    for t in thresholds:
        t = float(t)
        last = sum(1 for v in errs if v < t)          # torch.searchsorted, side='left'
        r = rec[:last] + [rec[last - 1]]
        x = errs[:last] + [t]
        area = sum((x[i + 1] - x[i]) * (r[i + 1] + r[i]) / 2 for i in range(len(x) - 1))
        out[f"AUC@{t}deg"] = area / t
    return out
