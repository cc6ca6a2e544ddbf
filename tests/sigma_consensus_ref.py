"""Float64 restatement of sigma-consensus scoring (openglue_amd.geometry with scoring="sigma", csrc/og_ransac.h,
csrc/sigma_consensus.hip) in numpy / scipy, on top of tests/geometry_ref.py and tests/homography_ref.py.

The definition is MAGSAC++'s with OpenCV's constants: n = 4 degrees of freedom, a = (n - 1) / 2, k = 3.64, sigma_max = threshold / k,
u_max = k^2 / 2.  With t = e / threshold^2 and u = t u_max,
    w(t) = (G(a, u) - G(a, u_max)) / (G(a) - G(a, u_max)),    q(t) = 1 - (g(a + 1, u) + u (G(a, u) - G(a, u_max))) / g(a + 1, u_max)
for 0 <= t <= 1 and 0 otherwise, G / g the unnormalised upper / lower incomplete gamma functions (scipy's gammaincc / gammainc times
gamma).  A model's quality is Q = sum of rint(65536 q(t_i)); the RANSAC loop, the draws, the solvers and the refits are the plain
restatements' with that score and with weighted normal equations."""
import math

import numpy as np
import torch
from scipy import special

from tests import geometry_ref as gref
from tests import homography_ref as href

A = 1.5
K = 3.64
U_MAX = K * K / 2
UNIT = 65536


def _G(a, x):
    return special.gammaincc(a, x) * special.gamma(a)


def _g(a, x):
    return special.gammainc(a, x) * special.gamma(a)


def _inside(t):
    t = np.asarray(t, dtype=np.float64)
    ok = (t >= 0) & (t <= 1)                                   # NaN compares false
    return ok, np.where(ok, t, 0.0) * U_MAX


def weight(t):
    ok, u = _inside(t)
    return np.where(ok, (_G(A, u) - _G(A, U_MAX)) / (special.gamma(A) - _G(A, U_MAX)), 0.0)


def quality(t):
    ok, u = _inside(t)
    return np.where(ok, 1.0 - (_g(A + 1, u) + u * (_G(A, u) - _G(A, U_MAX))) / _g(A + 1, U_MAX), 0.0)


def closed_G15(u):
    """G(1.5, u) = sqrt(u) exp(-u) + (sqrt(pi) / 2) erfc(sqrt u)"""
    u = np.asarray(u, dtype=np.float64)
    return np.sqrt(u) * np.exp(-u) + math.sqrt(math.pi) / 2 * special.erfc(np.sqrt(u))


def closed_g25(u):
    """g(2.5, u) = (3 sqrt(pi) / 4) erf(sqrt u) - exp(-u) (u^1.5 + 1.5 sqrt u)"""
    u = np.asarray(u, dtype=np.float64)
    return 0.75 * math.sqrt(math.pi) * special.erf(np.sqrt(u)) - np.exp(-u) * (u ** 1.5 + 1.5 * np.sqrt(u))


def match_t(e, t2):
    """Squared residuals e under the bound t2 -> (inlier mask e <= t2, t with 0 where the mask is false): a NaN or infinite e is no
    inlier, and a bound of 0 takes t = 0 for e = 0."""
    e = np.asarray(e, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        inl = e <= t2
    safe = np.where(inl, e, 0.0)
    return inl, (safe / t2 if t2 > 0 else np.zeros_like(safe))


def Q_of(e, t2):
    """The integer quality of a model with squared residuals e under the bound t2"""
    inl, t = match_t(e, t2)
    return int(np.rint(UNIT * quality(t))[inl].sum())


def Q_float(e, t2):
    """The same without the fixed-point rounding: sum of 65536 q"""
    inl, t = match_t(e, t2)
    return float((UNIT * quality(t))[inl].sum())


def weights_of(e, t2):
    inl, t = match_t(e, t2)
    return inl, np.where(inl, weight(t), 0.0)


# ------------------------------------------------------------------------------------------------ weighted fits
def eight_point_weighted(x0, x1, w):
    Arows = gref.constraint_rows(x0, x1)
    _, V = np.linalg.eigh((Arows * w[:, None]).T @ Arows)
    F = V[:, 0].reshape(3, 3)
    U, S, Vt = np.linalg.svd(F)
    F = U @ np.diag([S[0], S[1], 0.0]) @ Vt
    return F / np.linalg.norm(F)


def dlt_fit_weighted(x0, x1, w):
    Arows = href.dlt_rows(x0, x1)
    _, V = np.linalg.eigh((Arows * np.repeat(w, 2)[:, None]).T @ Arows)
    Hm = V[:, 0].reshape(3, 3)
    return Hm / np.linalg.norm(Hm)


# ------------------------------------------------------------------------------------------------ the whole procedures
def _ransac(n, min_n, refit_n, hypotheses, refine, models_of, residual, fit, t2):
    """The loop both models share.  models_of(h) -> the models of hypothesis h with their index; residual(model) -> e of every match;
    fit(weights, inlier mask) -> a refit.  Returns (model or None, Q, best index, Q of the winner before the refits)."""
    best_Q, best, best_model = -1, None, -1
    for h in range(hypotheses):
        for index, model in models_of(h):
            Q = Q_of(residual(model), t2)
            if Q > best_Q:
                best_Q, best, best_model = Q, model, index
    if best is None:
        return None, 0, -1, 0
    cur, cur_Q = best, best_Q
    for _ in range(refine):
        inl, w = weights_of(residual(cur), t2)
        if inl.sum() < refit_n:
            break
        new = fit(w[inl], inl)
        Qn = Q_of(residual(new), t2)
        if np.isfinite(new).all() and Qn >= cur_Q:
            cur, cur_Q = new, Qn
    return cur, cur_Q, best_model, best_Q


def fundamental_matrix_sigma(k0, k1, m0, nk=None, threshold=1.0, hypotheses=2048, refine=2, seed=0, pair=0):
    """One pair -> {'F' [3, 3] pixels, 'inliers' [M] bool (e <= threshold^2 under the final F), 'num_inliers', 'best_model'
    (hypothesis * 3 + solution in this basis's order, -1 without a model), 'Q' and 'quality' = Q / 65536 of the final model,
    'ransac_Q' (the winner's before the refits)}."""
    M = len(np.asarray(m0))
    idx, p0, p1 = gref.valid_matches(k0, k1, m0, nk)
    n = len(idx)
    none = {"F": np.zeros((3, 3)), "inliers": np.zeros(M, dtype=bool), "num_inliers": 0, "best_model": -1, "Q": 0, "quality": 0.0, "ransac_Q": 0}
    if n < 7:
        return none
    (c0, s0), (c1, s1) = gref.hartley(p0), gref.hartley(p1)
    x0, x1 = (p0 - c0) * s0, (p1 - c1) * s1
    t2 = threshold * threshold

    def models_of(h):
        pick = gref.draw_distinct(seed, pair, h, n)
        return [(h * 3 + s, F) for s, F in enumerate(gref.seven_point(x0[pick], x1[pick])[0])]
    residual = lambda F: gref.sampson_sq(F, x0, x1, s0, s1)
    F, Q, best_model, ransac_Q = _ransac(n, 7, 8, hypotheses, refine, models_of, residual, lambda w, inl: eight_point_weighted(x0[inl], x1[inl], w), t2)
    if F is None:
        return none
    mask = np.zeros(M, dtype=bool)
    inl = residual(F) <= t2
    mask[idx[inl]] = True
    return {"F": gref.to_pixels(F, c0, s0, c1, s1), "inliers": mask, "num_inliers": int(inl.sum()), "best_model": best_model, "Q": Q,
            "quality": Q / UNIT, "ransac_Q": ransac_Q}


def homography_sigma(k0, k1, m0, nk=None, threshold=3.0, hypotheses=2048, refine=2, seed=0, pair=0):
    """One pair -> {'H', 'inliers', 'num_inliers', 'best_model' (the hypothesis), 'Q', 'quality', 'ransac_Q'} as above."""
    M = len(np.asarray(m0))
    idx, p0, p1 = href.valid_matches(k0, k1, m0, nk)
    n = len(idx)
    none = {"H": np.zeros((3, 3)), "inliers": np.zeros(M, dtype=bool), "num_inliers": 0, "best_model": -1, "Q": 0, "quality": 0.0, "ransac_Q": 0}
    if n < 4:
        return none
    (c0, s0), (c1, s1) = href.hartley(p0), href.hartley(p1)
    x0, x1 = (p0 - c0) * s0, (p1 - c1) * s1
    t2 = threshold * threshold * s1 * s1

    def models_of(h):
        pick = href.draw_distinct(seed, pair, h, n, k=4)
        Hm = href.four_point(x0[pick], x1[pick])
        return [] if Hm is None else [(h, Hm)]
    residual = lambda Hm: href.transfer_sq(Hm, x0, x1)
    Hm, Q, best_model, ransac_Q = _ransac(n, 4, 5, hypotheses, refine, models_of, residual, lambda w, inl: dlt_fit_weighted(x0[inl], x1[inl], w), t2)
    if Hm is None:
        return none
    mask = np.zeros(M, dtype=bool)
    inl = residual(Hm) <= t2
    mask[idx[inl]] = True
    return {"H": href.to_pixels(Hm, c0, s0, c1, s1), "inliers": mask, "num_inliers": int(inl.sum()), "best_model": best_model, "Q": Q,
            "quality": Q / UNIT, "ransac_Q": ransac_Q}


def Q_of_pixel_F(F, k0, k1, m0, threshold, nk=None, rounded=True):
    """Q of a pixel-frame F over the pair's valid matches, in float64 (the Sampson error is the same in both frames)"""
    _, p0, p1 = gref.valid_matches(k0, k1, m0, nk)
    e = gref.sampson_sq(np.asarray(F, dtype=np.float64), p0, p1)
    return (Q_of if rounded else Q_float)(e, threshold * threshold)


def Q_of_pixel_H(Hm, k0, k1, m0, threshold, nk=None, rounded=True):
    _, p0, p1 = href.valid_matches(k0, k1, m0, nk)
    Hm = np.asarray(Hm, dtype=np.float64)
    e = href.transfer_sq(Hm, p0, p1) if Hm.any() else np.full(len(p0), np.inf)
    return (Q_of if rounded else Q_float)(e, threshold * threshold)


# ------------------------------------------------------------------------------------------------ the robustness experiment
PROPERTY_SEEDS = tuple(range(100, 108))
PROPERTY_THRESHOLDS = (1.0, 2.0, 4.0, 8.0, 16.0)
PROPERTY_H = 256


def property_scene(seed):
    """(k0, k1, m0 as numpy, true noise-free matches p0, p1 float64) of make_scene(1, 300, outliers=0.3, noise=0.5, seed): the same
    generator state without noise gives the clean positions, and the outlier mask tells which matches are true."""
    k0, k1, m0, tr, out = gref.make_scene(1, 300, outliers=0.3, noise=0.5, seed=seed)
    c0, c1, _, _, _ = gref.make_scene(1, 300, outliers=0.0, noise=0.0, seed=seed, dtype=torch.float64)
    good = ~out[0].numpy()
    return k0[0].numpy(), k1[0].numpy(), m0[0].numpy(), c0[0].numpy()[good], c1[0].numpy()[good]


def rms_sampson(F, p0, p1):
    """RMS Sampson distance (pixels) of the matches p0, p1 to the pixel-frame F; inf without a model"""
    F = np.asarray(F, dtype=np.float64)
    if not F.any():
        return math.inf
    return float(np.sqrt(gref.sampson_sq(F, p0, p1).mean()))
