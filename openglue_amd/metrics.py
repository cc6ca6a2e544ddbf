"""The validation metrics of the reference's training module on HIP kernels (utils/metrics.py, used by
models/matching_module.py:107-131):

  AccuracyUsingEpipolarDist   per-pair precision and matching score from the symmetric epipolar distance under the true E
  CameraPoseAUC               relative pose by five-point RANSAC + cheirality, pose error, AUC at the given thresholds
  relative_pose               the functional form of the pose estimate (poses, inliers, errors)

Thin wrappers over og_epipolar_precision / og_relative_pose (include/openglue_amd.h, csrc/metrics.hip); GPU tensors only.
Both classes keep the reference's constructor arguments, `update` signature, `compute()` keys and `reset()`, without
subclassing torchmetrics.  `update_batch` takes a whole SuperGlue.match batch (matches0 with -1 holes, ragged
num_keypoints0) in one call; a per-pair `update` runs the same kernels with B = 1.

Where the pose estimate deliberately differs from the reference's cv2.findEssentialMat(method=RANSAC, prob=0.99999):
  * every one of `hypotheses` samples is evaluated (no adaptive early stop; 1000 is cv2's iteration ceiling), and the samples
    come from a counter-based hash of (seed, pair, hypothesis), not from OpenCV's generator.  The pair index counts the pairs
    a metric has seen, so B per-pair updates draw exactly what one batched update of the same pairs draws;
  * the best model has the most inliers, ties going to the lowest (hypothesis, solution): outputs are bit-identical from run
    to run;
  * cheirality counts points in front of both cameras with the two-view linear depth of each inlier, not kornia's DLT
    triangulation (the same sign except for points at near-infinite depth);
  * the cosines of the rotation and translation errors are clamped to [-1, 1] (the reference's translation cosine is not,
    so there a value that rounds above 1 gives NaN).

The homography pre-training stage has no validation in the reference (OxfordParis1MDataModule has a train_dataloader only, and
pretrain_homography.py runs with num_sanity_val_steps=0).  Its items carry transformation['H'] instead of K0, K1, R, T, so the two
classes above cannot judge them; their perspective counterparts, over og_homography_precision / og_homography_corner_error
(csrc/homography.hip) and geometry.homography, can:

  HomographyAccuracy          precision and matching score from the transfer distance under the true H (pixels)
  HomographyAUC               a homography per pair by RANSAC, its mean corner error, AUC at the given thresholds (pixels)
  homography_precision, homography_error   their functional forms
"""
from __future__ import annotations

from typing import Dict, Sequence

import torch

from . import _lib, geometry

_TKEYS = ("K0", "K1", "R", "T")


def _batch(keypoints0, keypoints1, matches0, transformation, num_keypoints0):
    """Validate and convert one SuperGlue.match-shaped batch -> (B, M, N, tensors kept alive)."""
    k0 = _lib.gpu_tensor(keypoints0, "keypoints0", convert=True)
    k1 = _lib.gpu_tensor(keypoints1, "keypoints1", convert=True)
    m0 = _lib.gpu_tensor(matches0, "matches0", torch.int64, convert=True)
    if k0.dim() != 3 or k0.shape[2] != 2 or k1.dim() != 3 or k1.shape[2] != 2 or k1.shape[0] != k0.shape[0]:
        raise ValueError("keypoints0 / keypoints1 must be [B, M, 2] / [B, N, 2]")
    B, M, N = k0.shape[0], k0.shape[1], k1.shape[1]
    if tuple(m0.shape) != (B, M):
        raise ValueError(f"matches0 must be [B, M] = [{B}, {M}], got {list(m0.shape)}")
    t = {}
    for key in _TKEYS:
        v = _lib.gpu_tensor(transformation[key], f"transformation['{key}']", convert=True)
        want = (B, 3) if key == "T" else (B, 3, 3)
        if tuple(v.shape) != want:
            raise ValueError(f"transformation['{key}'] must be {list(want)}, got {list(v.shape)}")
        t[key] = v
    nk = None
    if num_keypoints0 is not None:
        nk = _lib.gpu_tensor(num_keypoints0, "num_keypoints0", torch.int32, convert=True)
        if tuple(nk.shape) != (B,):
            raise ValueError(f"num_keypoints0 must be [B] = [{B}]")
    return B, M, N, k0, k1, m0, t, nk


def epipolar_precision(keypoints0, keypoints1, matches0, transformation, num_keypoints0=None, threshold: float = 5e-4
                       ) -> Dict[str, torch.Tensor]:
    """utils/metrics.py:17-46 for a batch -> {'precision' [B], 'matching_score' [B] fp32, 'num_correct' [B] int32}."""
    B, M, N, k0, k1, m0, t, nk = _batch(keypoints0, keypoints1, matches0, transformation, num_keypoints0)
    dev = k0.device
    prec = torch.empty(B, device=dev, dtype=torch.float32)
    score = torch.empty(B, device=dev, dtype=torch.float32)
    correct = torch.empty(B, device=dev, dtype=torch.int32)
    _lib.call("og_epipolar_precision", dev, B, M, N, k0.data_ptr(), k1.data_ptr(), m0.data_ptr(), _lib.ptr(nk), t["K0"].data_ptr(),
              t["K1"].data_ptr(), t["R"].data_ptr(), t["T"].data_ptr(), float(threshold),
              prec.data_ptr(), score.data_ptr(), correct.data_ptr(), _lib.STREAM)
    return {"precision": prec, "matching_score": score, "num_correct": correct}


def relative_pose(keypoints0, keypoints1, matches0, transformation, ransac_inliers_threshold: float, num_keypoints0=None,
                  hypotheses: int = 1000, seed: int = 0, pair_offset: int = 0) -> Dict[str, torch.Tensor]:
    """The pose of CameraPoseAUC.update (utils/metrics.py:76-121) for a batch: RANSAC five-point essential matrix in calibrated
    space, cheirality choice, error against transformation['R'] / ['T'].  Returns {'R' [B, 3, 3], 't' [B, 3] (unit),
    'inliers' [B, M] bool, 'num_inliers' [B] int32, 'error' [B] degrees (inf with fewer than 5 matches or no model)}.
    `pair_offset` is added to the pair index the samples are drawn from."""
    B, M, N, k0, k1, m0, t, nk = _batch(keypoints0, keypoints1, matches0, transformation, num_keypoints0)
    hypotheses = int(hypotheses)
    if hypotheses <= 0:
        raise ValueError("hypotheses must be positive")
    dev = k0.device
    lib = _lib.load()
    nbytes = lib.og_relative_pose_workspace_bytes(B, M, hypotheses)
    if nbytes == 0:
        raise ValueError("unsupported relative_pose sizes")
    ws, wp = _lib.workspace(nbytes, dev)
    err = torch.empty(B, device=dev, dtype=torch.float32)
    Rp = torch.empty(B, 3, 3, device=dev, dtype=torch.float32)
    tp = torch.empty(B, 3, device=dev, dtype=torch.float32)
    inl = torch.empty(B, max(M, 1), device=dev, dtype=torch.uint8)
    ninl = torch.empty(B, device=dev, dtype=torch.int32)
    _lib.call("og_relative_pose", dev, B, M, N, k0.data_ptr(), k1.data_ptr(), m0.data_ptr(), _lib.ptr(nk), t["K0"].data_ptr(),
              t["K1"].data_ptr(), t["R"].data_ptr(), t["T"].data_ptr(), float(ransac_inliers_threshold),
              hypotheses, int(seed) & (2 ** 64 - 1), int(pair_offset), err.data_ptr(), Rp.data_ptr(),
              tp.data_ptr(), inl.data_ptr(), ninl.data_ptr(), wp, _lib.STREAM)
    return {"R": Rp, "t": tp, "inliers": inl[:, :M].bool(), "num_inliers": ninl, "error": err}


def essential_5pt(x0: torch.Tensor, x1: torch.Tensor):
    """The five-point minimal solver on its own: x0, x1 [count, 5, 2] calibrated correspondences (x1^T E x0 = 0) ->
    (E [count, 10, 3, 3] float64, unit Frobenius norm; num_solutions [count] int32).  Entries past num_solutions are undefined."""
    a = _lib.gpu_tensor(x0, "x0", torch.float64, convert=True)
    b = _lib.gpu_tensor(x1, "x1", torch.float64, convert=True)
    if a.dim() != 3 or a.shape[1:] != (5, 2) or b.shape != a.shape or a.shape[0] == 0:
        raise ValueError("x0 / x1 must both be [count, 5, 2] with count > 0")
    count = a.shape[0]
    dev = a.device
    E = torch.empty(count, 10, 3, 3, device=dev, dtype=torch.float64)
    ns = torch.empty(count, device=dev, dtype=torch.int32)
    _lib.call("og_essential_5pt", dev, count, a.data_ptr(), b.data_ptr(), E.data_ptr(), ns.data_ptr(), _lib.STREAM)
    return E, ns


def _single_pair(matched_kpts0, matched_kpts1, transformation, num_detected_kpts=None):
    """One pair as the reference passes it (compacted matches, a per-pair transformation) -> a B = 1 batch.  With
    num_detected_kpts the keypoints are padded to that many rows with -1 matches, so that matching_score divides by it."""
    kp0, kp1, m0, nk = _pad_pair(matched_kpts0, matched_kpts1, num_detected_kpts)
    tr = {key: _lib.gpu_tensor(transformation[key], f"transformation['{key}']", convert=True).unsqueeze(0) for key in _TKEYS}
    return kp0, kp1, m0, tr, nk


def _pad_pair(matched_kpts0, matched_kpts1, num_detected_kpts=None):
    """The keypoints and matches of _single_pair: (keypoints0 [1, M, 2], keypoints1 [1, K, 2], matches0 [1, M], num_keypoints0)."""
    k0 = _lib.gpu_tensor(matched_kpts0, "matched_kpts0", convert=True)
    k1 = _lib.gpu_tensor(matched_kpts1, "matched_kpts1", convert=True)
    if k0.dim() != 2 or k0.shape[1] != 2 or tuple(k1.shape) != tuple(k0.shape):
        raise ValueError("matched_kpts0 / matched_kpts1 must both be [K, 2]")
    K = k0.shape[0]
    dev = k0.device
    M = K if num_detected_kpts is None else max(int(num_detected_kpts), K)
    kp0 = torch.zeros(1, M, 2, device=dev, dtype=torch.float32)
    kp0[0, :K] = k0
    m0 = torch.full((1, M), -1, device=dev, dtype=torch.int64)
    m0[0, :K] = torch.arange(K, device=dev)
    nk = None if num_detected_kpts is None else torch.full((1,), int(num_detected_kpts), device=dev, dtype=torch.int32)
    return kp0, k1.unsqueeze(0), m0, nk


class AccuracyUsingEpipolarDist:
    """utils/metrics.py:10-51: mean precision and matching score over the pairs seen since the last reset()."""

    def __init__(self, threshold=5e-4):
        self.threshold = threshold
        self.reset()

    def reset(self):
        self.precision = []
        self.matching_score = []

    def update(self, matched_kpts0, matched_kpts1, transformation, num_detected_kpts):
        """One pair: matched keypoints [K, 2] of both images, transformation with K0, K1, R [3, 3] and T [3]."""
        self.update_batch(*_single_pair(matched_kpts0, matched_kpts1, transformation, num_detected_kpts))

    def update_batch(self, keypoints0, keypoints1, matches0, transformation, num_keypoints0=None):
        """A SuperGlue.match batch: keypoints0 [B, M, 2], keypoints1 [B, N, 2], matches0 [B, M] (-1: no match), batched
        transformation, num_keypoints0 [B] (None: M) -- the reference's num_detected_kpts."""
        r = epipolar_precision(keypoints0, keypoints1, matches0, transformation, num_keypoints0, self.threshold)
        self.precision.append(r["precision"])
        self.matching_score.append(r["matching_score"])

    def __call__(self, *args, **kwargs):
        self.update(*args, **kwargs)

    def compute(self):
        return {
            'Precision': torch.cat(self.precision).mean(),
            'Matching Score': torch.cat(self.matching_score).mean(),
        }


class CameraPoseAUC:
    """utils/metrics.py:55-141: relative pose per pair, AUC of the pose error at `auc_thresholds` (degrees)."""

    def __init__(self, auc_thresholds: Sequence[float], ransac_inliers_threshold: float, hypotheses: int = 1000, seed: int = 0):
        self.auc_thresholds = auc_thresholds
        self.ransac_inliers_threshold = ransac_inliers_threshold
        self.hypotheses = hypotheses
        self.seed = seed
        self.reset()

    def reset(self):
        self.pose_errors = []
        self._pairs = 0          # pairs seen: the pair index of the RANSAC draws

    def update(self, matched_kpts0, matched_kpts1, transformation):
        kp0, kp1, m0, tr, _ = _single_pair(matched_kpts0, matched_kpts1, transformation)
        self.update_batch(kp0, kp1, m0, tr)

    def update_batch(self, keypoints0, keypoints1, matches0, transformation, num_keypoints0=None):
        r = relative_pose(keypoints0, keypoints1, matches0, transformation, self.ransac_inliers_threshold, num_keypoints0,
                          self.hypotheses, self.seed, self._pairs)
        self._pairs += int(r["error"].shape[0])
        self.pose_errors.append(r["error"])

    def __call__(self, *args, **kwargs):
        self.update(*args, **kwargs)

    def compute(self):
        return pose_auc(torch.cat(self.pose_errors), self.auc_thresholds)


def _true_h(transformation, B: int) -> torch.Tensor:
    """transformation['H'] of a perspective item (pairs.homography_pairs: float32, image0 -> image1 in pixels) -> [B, 3, 3]"""
    s = geometry._shape(transformation["H"], "transformation['H']")
    if s != (B, 3, 3):
        raise ValueError(f"transformation['H'] must be {[B, 3, 3]}, got {list(s)}")
    return _lib.gpu_tensor(transformation["H"], "transformation['H']", convert=True)


def homography_precision(keypoints0, keypoints1, matches0, transformation, num_keypoints0=None, threshold: float = 3.0
                         ) -> Dict[str, torch.Tensor]:
    """The perspective counterpart of epipolar_precision: a match i is correct when |proj(transformation['H'], keypoints0[i]) -
    keypoints1[matches0[i]]| < threshold pixels (fp64) -> {'precision' [B] = correct / matched, 'matching_score' [B] = correct /
    num_keypoints0, both fp32 and 0 when nothing is matched, 'num_correct' [B] int32}.  Shapes as geometry.homography."""
    s0, s1, sm = (geometry._shape(t, n) for t, n in ((keypoints0, "keypoints0"), (keypoints1, "keypoints1"), (matches0, "matches0")))
    if len(s0) != 3 or s0[2] != 2 or len(s1) != 3 or s1[2] != 2 or s1[0] != s0[0] or s0[0] == 0:
        raise ValueError(f"keypoints0 / keypoints1 must be [B, M, 2] / [B, N, 2] with B > 0, got {list(s0)} / {list(s1)}")
    B, M, N = s0[0], s0[1], s1[1]
    if sm != (B, M):
        raise ValueError(f"matches0 must be [B, M] = [{B}, {M}], got {list(sm)}")
    if num_keypoints0 is not None and geometry._shape(num_keypoints0, "num_keypoints0") != (B,):
        raise ValueError(f"num_keypoints0 must be [B] = [{B}], got {list(num_keypoints0.shape)}")
    if not float(threshold) >= 0.0:
        raise ValueError(f"threshold must be non-negative, got {threshold}")
    Ht = _true_h(transformation, B)
    k0 = _lib.gpu_tensor(keypoints0, "keypoints0", convert=True)
    k1 = _lib.gpu_tensor(keypoints1, "keypoints1", convert=True)
    m0 = _lib.gpu_tensor(matches0, "matches0", torch.int64, convert=True)
    nk = None if num_keypoints0 is None else _lib.gpu_tensor(num_keypoints0, "num_keypoints0", torch.int32, convert=True)
    dev = k0.device
    prec = torch.empty(B, device=dev, dtype=torch.float32)
    score = torch.empty(B, device=dev, dtype=torch.float32)
    correct = torch.empty(B, device=dev, dtype=torch.int32)
    _lib.call("og_homography_precision", dev, B, M, N, k0.data_ptr(), k1.data_ptr(), m0.data_ptr(), _lib.ptr(nk), Ht.data_ptr(),
              float(threshold), prec.data_ptr(), score.data_ptr(), correct.data_ptr(), _lib.STREAM)
    return {"precision": prec, "matching_score": score, "num_correct": correct}


def homography_error(H_est, H_true, image_size) -> torch.Tensor:
    """Mean corner error: the four corners of an image of image_size = (width, height) mapped by H_est [B, 3, 3] (float64, as
    geometry.homography returns it; any scale) and by H_true [B, 3, 3] (float32) -> the mean distance in pixels [B] fp32, +inf for an
    all-zero estimate (no model) or a non-finite projection."""
    se, st = geometry._shape(H_est, "H_est"), geometry._shape(H_true, "H_true")
    if len(se) != 3 or se[1:] != (3, 3) or st != se or se[0] == 0:
        raise ValueError(f"H_est / H_true must both be [B, 3, 3] with B > 0, got {list(se)} / {list(st)}")
    width, height = (int(v) for v in image_size)
    if width <= 0 or height <= 0:
        raise ValueError(f"image_size must be (width, height) with both positive, got {image_size}")
    He = _lib.gpu_tensor(H_est, "H_est", torch.float64, convert=True)
    Ht = _lib.gpu_tensor(H_true, "H_true", convert=True)
    err = torch.empty(se[0], device=He.device, dtype=torch.float32)
    _lib.call("og_homography_corner_error", He.device, se[0], He.data_ptr(), Ht.data_ptr(), width, height, err.data_ptr(), _lib.STREAM)
    return err


class HomographyAccuracy:
    """AccuracyUsingEpipolarDist for perspective items (transformation['H']): mean precision and matching score, a match being
    correct within `threshold` pixels of where the true homography sends its keypoint."""

    def __init__(self, threshold=3.0):
        self.threshold = threshold
        self.reset()

    def reset(self):
        self.precision = []
        self.matching_score = []

    def update(self, matched_kpts0, matched_kpts1, transformation, num_detected_kpts):
        """One pair: matched keypoints [K, 2] of both images, transformation with H [3, 3]."""
        kp0, kp1, m0, nk = _pad_pair(matched_kpts0, matched_kpts1, num_detected_kpts)
        self.update_batch(kp0, kp1, m0, {"H": _lib.gpu_tensor(transformation["H"], "transformation['H']", convert=True).unsqueeze(0)}, nk)

    def update_batch(self, keypoints0, keypoints1, matches0, transformation, num_keypoints0=None):
        """A SuperGlue.match batch, as AccuracyUsingEpipolarDist.update_batch, with transformation['H'] [B, 3, 3]."""
        r = homography_precision(keypoints0, keypoints1, matches0, transformation, num_keypoints0, self.threshold)
        self.precision.append(r["precision"])
        self.matching_score.append(r["matching_score"])

    def __call__(self, *args, **kwargs):
        self.update(*args, **kwargs)

    def compute(self):
        return {
            'Precision': torch.cat(self.precision).mean(),
            'Matching Score': torch.cat(self.matching_score).mean(),
        }


class HomographyAUC:
    """CameraPoseAUC for perspective items: a homography per pair by geometry.homography (RANSAC threshold
    `ransac_inliers_threshold` pixels), its mean corner error against transformation['H'] over an image of image_size = (width,
    height), AUC of that error at `auc_thresholds` (pixels).  A pair without a model counts with an infinite error."""

    def __init__(self, auc_thresholds: Sequence[float], ransac_inliers_threshold: float, image_size, hypotheses: int = 2048, seed: int = 0):
        self.auc_thresholds = auc_thresholds
        self.ransac_inliers_threshold = ransac_inliers_threshold
        self.image_size = image_size
        self.hypotheses = hypotheses
        self.seed = seed
        self.reset()

    def reset(self):
        self.corner_errors = []
        self._pairs = 0          # pairs seen: the pair index of the RANSAC draws

    def update(self, matched_kpts0, matched_kpts1, transformation):
        kp0, kp1, m0, _ = _pad_pair(matched_kpts0, matched_kpts1)
        self.update_batch(kp0, kp1, m0, {"H": _lib.gpu_tensor(transformation["H"], "transformation['H']", convert=True).unsqueeze(0)})

    def update_batch(self, keypoints0, keypoints1, matches0, transformation, num_keypoints0=None):
        B = geometry._shape(keypoints0, "keypoints0")[0]
        Ht = _true_h(transformation, B)
        r = geometry.homography(keypoints0, keypoints1, matches0, num_keypoints0, threshold=self.ransac_inliers_threshold,
                                hypotheses=self.hypotheses, seed=self.seed, pair_offset=self._pairs)
        self._pairs += B
        self.corner_errors.append(homography_error(r["H"], Ht, self.image_size))

    def __call__(self, *args, **kwargs):
        self.update(*args, **kwargs)

    def compute(self):
        return {k[:-3] + "px": v for k, v in pose_auc(torch.cat(self.corner_errors), self.auc_thresholds).items()}      # 'AUC@{t}deg'


def pose_auc(errors: torch.Tensor, auc_thresholds: Sequence[float]) -> Dict[str, torch.Tensor]:
    """utils/metrics.py:125-141 as it stands: recall curve of the sorted errors, trapezoid area up to each threshold."""
    errors = torch.sort(errors).values
    recall = (torch.arange(len(errors), device=errors.device) + 1) / len(errors)
    zero = torch.zeros(1, device=errors.device)
    errors = torch.cat([zero, errors])
    recall = torch.cat([zero, recall])

    aucs = {}
    for threshold in auc_thresholds:
        threshold = torch.tensor(threshold).to(errors.device)
        last_index = torch.searchsorted(errors, threshold)
        r = torch.cat([recall[:last_index], recall[last_index - 1].unsqueeze(0)])
        e = torch.cat([errors[:last_index], threshold.unsqueeze(0)])
        area = torch.trapz(r, x=e) / threshold
        aucs[f'AUC@{threshold}deg'] = area
    return aucs
