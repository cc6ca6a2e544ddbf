"""Uncalibrated geometric verification on HIP kernels: the last step of the reference's inference.py, which takes the matches to
cv2.findFundamentalMat(keypoints0, keypoints1, cv2.USAC_MAGSAC, 1.0, 0.999, 100000) and keeps the inliers (inference.py:214-235).

  fundamental_matrix   a whole SuperGlue.match batch (matches0 with -1 holes, ragged num_keypoints0) -> F, inlier mask, counts
  find_fundamental     one pair of compacted matches -> (F, inliers), cv2's return order
  fundamental_7pt      the seven-point minimal solver on its own

Thin wrappers over og_fundamental_matrix / og_fundamental_7pt (include/openglue_amd.h, csrc/geometry.hip); GPU tensors only, no
host synchronisation.  Per pair: Hartley normalisation of the valid matches, `hypotheses` seven-point samples drawn by a
counter-based hash of (seed, pair_offset + pair, hypothesis), every model (up to 3 per sample) scored by its number of matches with
squared Sampson error <= threshold^2 (pixels), the winner by most inliers and lowest (hypothesis, solution) on ties, then `refine`
normalised eight-point refits on the inliers, each kept if it loses no inlier.  Outputs are bit-identical from run to run, and B
calls of one pair with pair_offset = b give what one batched call gives.

Where this deliberately differs from cv2.USAC_MAGSAC:
  * the default scoring="inliers" counts: `threshold` is a plain inlier threshold on the Sampson error.  scoring="sigma" reproduces
    MAGSAC++'s sigma-consensus scoring and its weighted refit (below); USAC's adaptive stop, its local-optimisation schedule and its
    degeneracy test are still not reproduced;
  * the sample count is fixed: every one of `hypotheses` samples is evaluated, there is no adaptive stop (2048 gives 0.999
    confidence down to an inlier ratio of about 0.45: ln 0.001 / ln(1 - 0.45^7) ~ 1850);
  * the random draws are the hash's, not OpenCV's generator;
  * there is no degeneracy test for planar scenes or dominant planes: for such input F is whatever the data support (a homography
    leaves a family of F that fit equally well), and the mask is still finite and deterministic.
With fewer than 7 valid matches, or no surviving model, F is zero, no match is an inlier and best_model is -1 (cv2 returns None).

scoring="sigma" (fundamental_matrix, find_fundamental, homography, find_homography; og_fundamental_matrix_sc / og_homography_sc,
in the same two units) marginalises over the noise scale up to sigma_max = threshold / 3.64, with OpenCV's constants (4 degrees of
freedom, a = 1.5, u_max = 3.64^2 / 2).  With e a match's squared residual, t = e / threshold^2 and u = t u_max:
  w(t) = (G(a, u) - G(a, u_max)) / (G(a) - G(a, u_max)),   q(t) = 1 - (g(a + 1, u) + u (G(a, u) - G(a, u_max))) / g(a + 1, u_max)
for t <= 1 (G / g: upper / lower incomplete gamma), 0 otherwise.  A model's score is Q = sum of rint(65536 q(t)) over the valid
matches, an integer, so the winner is independent of the summation order; the refits weigh each match's rows by w(t) and are kept
when Q does not drop; 'inliers' and 'num_inliers' keep their meaning (e <= threshold^2 under the final model) and 'quality' is
Q / 65536, the soft inlier count.  `threshold` is then an upper bound on the noise rather than a decision boundary: a generous one
costs little (8 px where the noise is 0.5 px loses nothing), one below about twice the noise makes the weights too tight and is
worse than counting (DESIGN 4.10c has the figures).  sigma_consensus(t) evaluates q and w as the kernels do.

Planar scenes, and the pairs of the homography pre-training stage, get the same treatment with the homography as the model
(cv2.findHomography(keypoints0, keypoints1, cv2.RANSAC, 3.0)):

  homography           a whole SuperGlue.match batch -> H, inlier mask, counts
  find_homography      one pair of compacted matches -> (H / H[2, 2], inliers), cv2's return order
  homography_4pt       the four-point minimal solver on its own

over og_homography / og_homography_4pt (csrc/homography.hip).  Per pair: the same normalisation and draws with 4 matches per sample,
at most one model per sample, scored by its number of matches with squared forward transfer error |proj(H, x0) - x1|^2 <=
threshold^2 (pixels), the winner by most inliers and the lowest hypothesis on ties, then `refine` normalised DLT refits on the
inliers, each kept if it loses no inlier.  Where this deliberately differs from cv2.findHomography(..., cv2.RANSAC):
  * the sample count is fixed and the draws are the hash's, as above (2048 samples of 4 give 0.999 confidence down to an inlier
    ratio of about 0.25);
  * a sample is rejected by cv2's orientation test on its four point triples, which here also rejects a collinear triple;
  * the refits are linear least squares (DLT) on the inliers; there is no Levenberg-Marquardt polish of the reprojection error.
With fewer than 4 valid matches, or no surviving model, H is zero, no match is an inlier and best_model is -1.
"""
from __future__ import annotations

from typing import Dict, Tuple

import torch

from . import _lib


def _shape(t, name: str) -> Tuple[int, ...]:
    """The shape of a tensor argument; anything else gets gpu_tensor's refusal.  Shapes and scalar arguments are checked before the
    device, so a bad call fails the same way wherever its tensors live."""
    if not isinstance(t, torch.Tensor):
        _lib.gpu_tensor(t, name)
    return tuple(t.shape)


SIGMA_MAX_MATCHES = 32768      # og_fundamental_matrix_sc / og_homography_sc: Q + 1 must fit 32 bits


def _sigma(scoring) -> bool:
    """scoring -> whether it is "sigma"; anything but "inliers" and "sigma" is refused before any device work."""
    if scoring not in ("inliers", "sigma"):
        raise ValueError(f"scoring must be 'inliers' or 'sigma', got {scoring!r}")
    return scoring == "sigma"


def _ransac(key, entry, ws_entry, models, keypoints0, keypoints1, matches0, num_keypoints0, threshold, hypotheses, refine, seed, pair_offset,
            scoring) -> Dict[str, torch.Tensor]:
    """The batched call of fundamental_matrix (key "F", 3 models per sample) and homography (key "H", 1): the checks, the workspace of
    `ws_entry`, and `entry` or, with scoring="sigma", `entry`_sc, which takes `quality` as well."""
    sigma = _sigma(scoring)
    s0, s1, sm = _shape(keypoints0, "keypoints0"), _shape(keypoints1, "keypoints1"), _shape(matches0, "matches0")
    if len(s0) != 3 or s0[2] != 2 or len(s1) != 3 or s1[2] != 2 or s1[0] != s0[0] or s0[0] == 0:
        raise ValueError(f"keypoints0 / keypoints1 must be [B, M, 2] / [B, N, 2] with B > 0, got {list(s0)} / {list(s1)}")
    B, M, N = s0[0], s0[1], s1[1]
    if sm != (B, M):
        raise ValueError(f"matches0 must be [B, M] = [{B}, {M}], got {list(sm)}")
    if num_keypoints0 is not None and _shape(num_keypoints0, "num_keypoints0") != (B,):
        raise ValueError(f"num_keypoints0 must be [B] = [{B}], got {list(num_keypoints0.shape)}")
    hypotheses, refine = int(hypotheses), int(refine)
    if hypotheses <= 0 or refine < 0 or not float(threshold) >= 0.0:
        raise ValueError(f"hypotheses must be positive, refine and threshold non-negative, got {hypotheses}, {refine}, {threshold}")
    if models * B * hypotheses > 2 ** 30:
        per = f"{models} * " if models > 1 else ""
        raise ValueError(f"{per}batch * hypotheses must not exceed 2^30, got {per}{B} * {hypotheses}")
    if sigma and M > SIGMA_MAX_MATCHES:
        raise ValueError(f"scoring='sigma' takes at most {SIGMA_MAX_MATCHES} keypoints per image, got M = {M}")
    k0 = _lib.gpu_tensor(keypoints0, "keypoints0", convert=True)
    k1 = _lib.gpu_tensor(keypoints1, "keypoints1", convert=True)
    m0 = _lib.gpu_tensor(matches0, "matches0", torch.int64, convert=True)
    nk = None if num_keypoints0 is None else _lib.gpu_tensor(num_keypoints0, "num_keypoints0", torch.int32, convert=True)
    dev = k0.device
    ws, wp = _lib.workspace(getattr(_lib.load(), ws_entry)(B, M, hypotheses), dev)      # sizes checked above
    model = torch.empty(B, 3, 3, device=dev, dtype=torch.float64)
    inl = torch.empty(B, max(M, 1), device=dev, dtype=torch.uint8)
    ninl = torch.empty(B, device=dev, dtype=torch.int32)
    best = torch.empty(B, device=dev, dtype=torch.int32)
    r = {key: model, "inliers": inl, "num_inliers": ninl, "best_model": best}
    if sigma:
        r["quality"] = torch.empty(B, device=dev, dtype=torch.float32)
    _lib.call(entry + "_sc" if sigma else entry, dev, B, M, N, k0.data_ptr(), k1.data_ptr(), m0.data_ptr(), _lib.ptr(nk), float(threshold),
              hypotheses, refine, int(seed) & (2 ** 64 - 1), int(pair_offset), model.data_ptr(), inl.data_ptr(), ninl.data_ptr(),
              best.data_ptr(), *([r["quality"].data_ptr()] if sigma else []), wp, _lib.STREAM)
    r["inliers"] = inl[:, :M].bool()
    return r


def _find(batched, matched_kpts0, matched_kpts1, kw) -> Dict[str, torch.Tensor]:
    """One pair of compacted matches [K, 2] / [K, 2] through `batched` (fundamental_matrix or homography) as a batch of one."""
    _sigma(kw.get("scoring", "inliers"))
    s0, s1 = _shape(matched_kpts0, "matched_kpts0"), _shape(matched_kpts1, "matched_kpts1")
    if len(s0) != 2 or s0[1] != 2 or s1 != s0:
        raise ValueError(f"matched_kpts0 / matched_kpts1 must both be [K, 2], got {list(s0)} / {list(s1)}")
    k0 = _lib.gpu_tensor(matched_kpts0, "matched_kpts0", convert=True)
    k1 = _lib.gpu_tensor(matched_kpts1, "matched_kpts1", convert=True)
    m0 = torch.arange(k0.shape[0], device=k0.device).unsqueeze(0)
    return batched(k0.unsqueeze(0), k1.unsqueeze(0), m0, **kw)


def _minimal(entry, sample, models, x0, x1):
    """A minimal solver on its own: x0, x1 [count, sample, 2] -> (models [count, (models,) 3, 3] float64, num_solutions [count] int32)."""
    s0, s1 = _shape(x0, "x0"), _shape(x1, "x1")
    if len(s0) != 3 or s0[1:] != (sample, 2) or s1 != s0 or not 0 < s0[0] <= 2 ** 30:
        raise ValueError(f"x0 / x1 must both be [count, {sample}, 2] with 0 < count <= 2^30, got {list(s0)} / {list(s1)}")
    a = _lib.gpu_tensor(x0, "x0", torch.float64, convert=True)
    b = _lib.gpu_tensor(x1, "x1", torch.float64, convert=True)
    count = a.shape[0]
    dev = a.device
    out = torch.empty(count, *([models] if models > 1 else []), 3, 3, device=dev, dtype=torch.float64)
    ns = torch.empty(count, device=dev, dtype=torch.int32)
    _lib.call(entry, dev, count, a.data_ptr(), b.data_ptr(), out.data_ptr(), ns.data_ptr(), _lib.STREAM)
    return out, ns


def fundamental_matrix(keypoints0, keypoints1, matches0, num_keypoints0=None, threshold: float = 1.0, hypotheses: int = 2048,
                       refine: int = 2, seed: int = 0, pair_offset: int = 0, scoring: str = "inliers") -> Dict[str, torch.Tensor]:
    """keypoints0 [B, M, 2], keypoints1 [B, N, 2] (pixels), matches0 [B, M] (-1 or outside [0, N): no match), num_keypoints0 [B]
    (None: M) -> {'F' [B, 3, 3] float64 in pixels with x1^T F x0 = 0, unit Frobenius norm, largest entry positive; 'inliers' [B, M]
    bool at the positions of keypoints0; 'num_inliers' [B] int32; 'best_model' [B] int32 = hypothesis * 3 + solution of the RANSAC
    winner, -1 without one}.  `threshold` in pixels; `refine` least-squares rounds (0: the minimal model as it is).  scoring="sigma":
    sigma-consensus scoring and weighted refits (module docstring), M <= 32768, and 'quality' [B] float32 joins the dict."""
    return _ransac("F", "og_fundamental_matrix", "og_fundamental_matrix_workspace_bytes", 3, keypoints0, keypoints1, matches0, num_keypoints0,
                   threshold, hypotheses, refine, seed, pair_offset, scoring)


def find_fundamental(matched_kpts0, matched_kpts1, **kw) -> Tuple[torch.Tensor, torch.Tensor]:
    """One pair as inference.py passes it to cv2.findFundamentalMat: matched keypoints [K, 2] of both images -> (F [3, 3] float64,
    inliers [K] bool).  Keyword arguments as fundamental_matrix (threshold, hypotheses, refine, seed, pair_offset, scoring)."""
    r = _find(fundamental_matrix, matched_kpts0, matched_kpts1, kw)
    return r["F"][0], r["inliers"][0]


def fundamental_7pt(x0: torch.Tensor, x1: torch.Tensor):
    """The seven-point minimal solver on its own: x0, x1 [count, 7, 2] correspondences (x1^T F x0 = 0) with coordinates of order 1
    -> (F [count, 3, 3, 3] float64, unit Frobenius norm, zero past num_solutions; num_solutions [count] int32, 0..3)."""
    return _minimal("og_fundamental_7pt", 7, 3, x0, x1)


def homography(keypoints0, keypoints1, matches0, num_keypoints0=None, threshold: float = 3.0, hypotheses: int = 2048,
               refine: int = 2, seed: int = 0, pair_offset: int = 0, scoring: str = "inliers") -> Dict[str, torch.Tensor]:
    """keypoints0 [B, M, 2], keypoints1 [B, N, 2] (pixels), matches0 [B, M] (-1 or outside [0, N): no match), num_keypoints0 [B]
    (None: M) -> {'H' [B, 3, 3] float64 in pixels with x1 ~ H x0, unit Frobenius norm, largest entry positive; 'inliers' [B, M]
    bool at the positions of keypoints0; 'num_inliers' [B] int32; 'best_model' [B] int32 = hypothesis of the RANSAC winner, -1
    without one}.  `threshold` in pixels; `refine` least-squares rounds (0: the minimal model as it is).  scoring="sigma":
    sigma-consensus scoring and weighted refits (module docstring), M <= 32768, and 'quality' [B] float32 joins the dict."""
    return _ransac("H", "og_homography", "og_homography_workspace_bytes", 1, keypoints0, keypoints1, matches0, num_keypoints0, threshold,
                   hypotheses, refine, seed, pair_offset, scoring)


def find_homography(matched_kpts0, matched_kpts1, **kw) -> Tuple[torch.Tensor, torch.Tensor]:
    """One pair as a caller passes it to cv2.findHomography: matched keypoints [K, 2] of both images -> (H [3, 3] float64 divided by
    H[2, 2] as cv2 returns it, zero without a model; inliers [K] bool).  Keyword arguments as homography (threshold, hypotheses,
    refine, seed, pair_offset, scoring).  An H whose last entry is 0 (the origin sent to infinity) has no such form and comes out non-finite."""
    r = _find(homography, matched_kpts0, matched_kpts1, kw)
    H = r["H"][0]
    return torch.where(r["best_model"][0] >= 0, H / H[2, 2], torch.zeros_like(H)), r["inliers"][0]      # no host synchronisation


def homography_4pt(x0: torch.Tensor, x1: torch.Tensor):
    """The four-point minimal solver on its own: x0, x1 [count, 4, 2] correspondences (x1 ~ H x0) with coordinates of order 1
    -> (H [count, 3, 3] float64, unit Frobenius norm, largest entry positive, zero without a solution; num_solutions [count] int32,
    0 or 1)."""
    return _minimal("og_homography_4pt", 4, 1, x0, x1)


def sigma_consensus(t: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """The sigma-consensus quality and weight as the kernels evaluate them (og_sigma_consensus_eval): t = e / threshold^2, any shape,
    float32 -> (q int64 in units of 2^-16, i.e. rint(65536 q(t)) within one unit and non-increasing in t; w float32).  Both are 0 for
    t outside [0, 1] and for NaN; t = 0 gives (65536, 1)."""
    shape = _shape(t, "t")
    count = 1
    for d in shape:
        count *= d
    if not 0 < count <= 2 ** 30:
        raise ValueError(f"t must hold between 1 and 2^30 values, got {list(shape)}")
    a = _lib.gpu_tensor(t, "t", convert=True)
    q = torch.empty(count, device=a.device, dtype=torch.int32)
    w = torch.empty(count, device=a.device, dtype=torch.float32)
    _lib.call("og_sigma_consensus_eval", a.device, count, a.data_ptr(), q.data_ptr(), w.data_ptr(), _lib.STREAM)
    return q.to(torch.int64).reshape(shape), w.reshape(shape)
