"""Float64 restatement of the homography path (openglue_amd.geometry.homography, openglue_amd.metrics.homography_precision /
homography_error, csrc/homography.hip) in numpy, and the planar scenes its tests use.

The procedure is the kernels': Hartley normalisation of the valid matches, the same counter-based draws (tests/geometry_ref.py with
k = 4, so hypothesis h of pair p picks the same four matches), the four-point solver with its validity rule, transfer-error counting
in pixels, most inliers with the lowest hypothesis on ties, and the DLT refit rounds with their accept rule.  The arithmetic is
independent: the null vector of the DLT system comes from an SVD (minimal sample) or eigh (refit), where the kernel eliminates and
runs Jacobi; everything is float64, where the kernel scores in fp32."""
import numpy as np
import torch

from tests.geometry_ref import draw_distinct, hartley, mix64, valid_matches      # noqa: F401 (re-exported for the tests)

AREA_EPS = 1e-9
TRIPLES = ((1, 2, 3), (0, 2, 3), (0, 1, 3), (0, 1, 2))


# ------------------------------------------------------------------------------------------------ pieces
def project(H, p):
    """p [n, 2] under H [3, 3] -> [n, 2]; a point on the line sent to infinity gives inf or NaN"""
    p = np.asarray(p, dtype=np.float64)
    h = np.concatenate([p, np.ones((len(p), 1))], 1) @ np.asarray(H, dtype=np.float64).T
    with np.errstate(divide="ignore", invalid="ignore"):
        return h[:, :2] / h[:, 2:3]


def transfer_sq(H, p0, p1):
    """Squared forward transfer error |proj(H, p0) - p1|^2 in the units of the points; non-finite -> inf (an outlier)."""
    with np.errstate(invalid="ignore", over="ignore"):
        d = ((project(H, p0) - np.asarray(p1, dtype=np.float64)) ** 2).sum(1)
    return np.where(np.isfinite(d), d, np.inf)


def dlt_rows(x0, x1):
    """Two rows per correspondence: (x0^T, 0, -u1 x0^T), (0, x0^T, -v1 x0^T) -> [2 n, 9], the pair of a match adjacent"""
    x0, x1 = np.asarray(x0, dtype=np.float64), np.asarray(x1, dtype=np.float64)
    n = len(x0)
    h0 = np.concatenate([x0, np.ones((n, 1))], 1)
    A = np.zeros((2 * n, 9))
    A[0::2, 0:3] = h0
    A[0::2, 6:9] = -x1[:, 0:1] * h0
    A[1::2, 3:6] = h0
    A[1::2, 6:9] = -x1[:, 1:2] * h0
    return A


def signed_area2(x, i, j, k):
    return (x[j, 0] - x[i, 0]) * (x[k, 1] - x[i, 1]) - (x[j, 1] - x[i, 1]) * (x[k, 0] - x[i, 0])


def sample_is_oriented(x0, x1):
    """Rule (a): every triple has a signed area above AREA_EPS in both images, of the same sign in both."""
    for t in TRIPLES:
        a0, a1 = signed_area2(x0, *t), signed_area2(x1, *t)
        if not (abs(a0) > AREA_EPS and abs(a1) > AREA_EPS and (a0 > 0) == (a1 > 0)):
            return False
    return True


def unit_signed(H):
    H = H / np.linalg.norm(H)
    return -H if H.reshape(9)[np.abs(H).argmax()] < 0 else H


def four_point(x0, x1):
    """x0, x1 [4, 2] of order 1 -> the unit-norm H [3, 3] with its largest entry positive, or None by the rules (a)-(c)."""
    x0, x1 = np.asarray(x0, dtype=np.float64), np.asarray(x1, dtype=np.float64)
    if not (np.isfinite(x0).all() and np.isfinite(x1).all()) or not sample_is_oriented(x0, x1):
        return None
    A = dlt_rows(x0, x1)
    H = np.linalg.svd(A)[2][8].reshape(3, 3)
    if not np.isfinite(H).all() or not np.linalg.norm(H) > 0:
        return None
    H = unit_signed(H)
    if not np.abs(A @ H.reshape(9)).max() <= 1e-9:
        return None
    return H


def dlt_fit(x0, x1):
    """Least-squares H through normalised correspondences, unit norm."""
    A = dlt_rows(x0, x1)
    _, V = np.linalg.eigh(A.T @ A)
    H = V[:, 0].reshape(3, 3)
    return H / np.linalg.norm(H)


def to_pixels(Hn, c0, s0, c1, s1):
    T0 = np.array([[s0, 0, -s0 * c0[0]], [0, s0, -s0 * c0[1]], [0, 0, 1.0]])
    T1 = np.array([[s1, 0, -s1 * c1[0]], [0, s1, -s1 * c1[1]], [0, 0, 1.0]])
    return unit_signed(np.linalg.inv(T1) @ Hn @ T0)


# ------------------------------------------------------------------------------------------------ the whole procedure
def homography(k0, k1, m0, nk=None, threshold=3.0, hypotheses=2048, refine=2, seed=0, pair=0):
    """One pair -> {'H' [3, 3] pixels, 'inliers' [M] bool, 'num_inliers', 'best_model' (the hypothesis, -1 without a model),
    'ransac_inliers' (the winner's count before the refits)}."""
    M = len(np.asarray(m0))
    idx, p0, p1 = valid_matches(k0, k1, m0, nk)
    n = len(idx)
    none = {"H": np.zeros((3, 3)), "inliers": np.zeros(M, dtype=bool), "num_inliers": 0, "best_model": -1, "ransac_inliers": 0}
    if n < 4:
        return none
    (c0, s0), (c1, s1) = hartley(p0), hartley(p1)
    x0, x1 = (p0 - c0) * s0, (p1 - c1) * s1
    t2 = threshold * threshold * s1 * s1
    best, best_H, best_model = -1, None, -1
    for h in range(hypotheses):
        pick = draw_distinct(seed, pair, h, n, k=4)
        Hm = four_point(x0[pick], x1[pick])
        if Hm is None:
            continue
        cnt = int((transfer_sq(Hm, x0, x1) <= t2).sum())
        if cnt > best:
            best, best_H, best_model = cnt, Hm, h
    if best_H is None:
        return none
    Hc, cur = best_H, best
    for _ in range(refine):
        if cur < 5:
            break
        inl = transfer_sq(Hc, x0, x1) <= t2
        Hn = dlt_fit(x0[inl], x1[inl])
        cnt = int((transfer_sq(Hn, x0, x1) <= t2).sum())
        if np.isfinite(Hn).all() and cnt >= cur:
            Hc, cur = Hn, cnt
    mask = np.zeros(M, dtype=bool)
    mask[idx[transfer_sq(Hc, x0, x1) <= t2]] = True
    return {"H": to_pixels(Hc, c0, s0, c1, s1), "inliers": mask, "num_inliers": cur, "best_model": best_model, "ransac_inliers": best}


# ------------------------------------------------------------------------------------------------ metrics
def precision(k0, k1, m0, H_true, nk=None, threshold=3.0):
    """One pair -> (precision, matching_score as float32, num_correct, the distances of the valid matches in float64).  H_true is
    taken as float32 values, as the kernel receives it."""
    idx, p0, p1 = valid_matches(k0, k1, m0, nk)
    Ht = np.asarray(H_true, dtype=np.float32).astype(np.float64)
    with np.errstate(invalid="ignore"):
        d = np.sqrt(((project(Ht, p0) - p1) ** 2).sum(1))
    correct = int((d < float(np.float32(threshold))).sum())
    M = len(np.asarray(m0))
    det = M if nk is None else min(int(nk), M)
    if len(idx) == 0:
        return np.float32(0), np.float32(0), 0, d
    return np.float32(correct) / np.float32(len(idx)), np.float32(correct) / np.float32(det), correct, d


def corner_error(H_est, H_true, width, height):
    """Mean distance of the four image corners under both maps; inf for an all-zero estimate or a non-finite projection."""
    H_est = np.asarray(H_est, dtype=np.float64)
    if not H_est.any():
        return np.inf
    c = np.array([[0, 0], [0, height - 1], [width - 1, 0], [width - 1, height - 1]], dtype=np.float64)
    with np.errstate(invalid="ignore"):
        e = np.sqrt(((project(H_est, c) - project(np.asarray(H_true, dtype=np.float64), c)) ** 2).sum(1)).mean()
    return float(e) if np.isfinite(e) else np.inf


# ------------------------------------------------------------------------------------------------ scenes
W, H = 640, 480
OUT_SEP = 30.0      # outliers lie at least this many thresholds from where the true homography sends their keypoint
MAX_SHIFT = 64.0    # the corners of the image move by up to this much in each coordinate


def perspective_from_corners(src, dst):
    """The homography through four correspondences with H[2, 2] = 1 (the 8 x 8 system of tests/pairs_ref.py), float64."""
    A, b = np.zeros((8, 8)), np.zeros(8)
    for i in range(4):
        (x, y), (u, v) = src[i], dst[i]
        A[i] = [x, y, 1, 0, 0, 0, -x * u, -y * u]
        A[i + 4] = [0, 0, 0, x, y, 1, -x * v, -y * v]
        b[i], b[i + 4] = u, v
    return np.append(np.linalg.solve(A, b), 1.0).reshape(3, 3)


def make_scene(B, n, outliers=0.0, noise=0.0, seed=0, thr_px=3.0, dtype=torch.float32):
    """B pairs of n matches at 640 x 480 (keypoints0 [B, n, 2], keypoints1 [B, n, 2] in `dtype`, matches0 = identity), float64 truth
    on the CPU: the true H maps the four image corners to themselves displaced by up to +-MAX_SHIFT px in each coordinate (the
    construction of tests/pairs_ref.py; the quadrilateral stays convex, so orientation is preserved), keypoints0 uniform in the
    image, keypoints1 = proj(H, keypoints0); outliers are keypoints1 moved at least OUT_SEP thresholds from there.
    Returns (k0, k1, matches0, H_true [B, 3, 3] float64, outlier mask)."""
    g = torch.Generator().manual_seed(seed)
    k0 = torch.zeros(B, n, 2, dtype=torch.float64)
    k1 = torch.zeros(B, n, 2, dtype=torch.float64)
    Hs = torch.zeros(B, 3, 3, dtype=torch.float64)
    out_mask = torch.zeros(B, n, dtype=torch.bool)
    size = torch.tensor([W - 1.0, H - 1.0], dtype=torch.float64)
    src = np.array([[0, 0], [0, H - 1], [W - 1, 0], [W - 1, H - 1]], dtype=np.float64)
    for b in range(B):
        shift = (2 * torch.rand(4, 2, generator=g, dtype=torch.float64) - 1) * MAX_SHIFT
        Ht = perspective_from_corners(src, src + shift.numpy())
        p0 = torch.rand(n, 2, generator=g, dtype=torch.float64) * size
        true1 = torch.from_numpy(project(Ht, p0.numpy()))
        p1 = true1.clone()
        if noise:
            p0 = p0 + noise * torch.randn(n, 2, generator=g, dtype=torch.float64)
            p1 = p1 + noise * torch.randn(n, 2, generator=g, dtype=torch.float64)
        n_out = int(round(outliers * n))
        if n_out:
            idx = torch.randperm(n, generator=g)[:n_out]
            todo = torch.ones(n_out, dtype=torch.bool)
            for _ in range(100):
                c = torch.rand(n_out, 2, generator=g, dtype=torch.float64) * size
                ok = todo & (((c - true1[idx]) ** 2).sum(1) > (OUT_SEP * thr_px) ** 2)
                p1[idx[ok]] = c[ok]
                todo &= ~ok
            idx = idx[~todo]
            out_mask[b, idx] = True
        k0[b], k1[b], Hs[b] = p0, p1, torch.from_numpy(Ht)
    return k0.to(dtype), k1.to(dtype), torch.arange(n).repeat(B, 1), Hs, out_mask
