"""Float64 restatement of the reference's utils/metrics.py formulas (and the kornia 0.6 functions it calls), for the tests of
openglue_amd.metrics.  Torch ops on CPU tensors, one pair at a time unless a function says otherwise."""
import math

import numpy as np
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


# ------------------------------------------------------------------------------------------------ five-point solver, numpy
# Independent of csrc/metrics.hip in its arithmetic: the null space comes from an SVD (any basis, no chart singled out), the ten
# cubics are multiplied out as dense exponent arrays, their leading block is solved by LU, and the solutions are the eigenvectors of
# the 10 x 10 multiplication-by-x matrix (Stewenius), where the kernel eliminates by hand, hides z and bisects a Sturm sequence.
_DEG3 = [(3, 0, 0), (2, 1, 0), (2, 0, 1), (1, 2, 0), (1, 1, 1), (1, 0, 2), (0, 3, 0), (0, 2, 1), (0, 1, 2), (0, 0, 3)]
_BASIS = [(2, 0, 0), (1, 1, 0), (1, 0, 1), (0, 2, 0), (0, 1, 1), (0, 0, 2), (1, 0, 0), (0, 1, 0), (0, 0, 1), (0, 0, 0)]


def _pmul3(a, b):
    """Product of two polynomials in (x, y, z) held as arrays indexed by the exponents."""
    out = np.zeros(tuple(sa + sb - 1 for sa, sb in zip(a.shape, b.shape)))
    for i, j, k in zip(*np.nonzero(a)):
        out[i:i + b.shape[0], j:j + b.shape[1], k:k + b.shape[2]] += a[i, j, k] * b
    return out


def essential_constraints(E):
    """The ten constraints of an essential matrix: 2 E E^T E - tr(E E^T) E (9) and det E."""
    EEt = E @ E.T
    return np.concatenate([(2 * EEt @ E - np.trace(EEt) * E).reshape(9), [np.linalg.det(E)]])


def _constraint_jacobian(E, basis):
    """d constraints / d (x, y, z) at E = x X + y Y + z Z + W, analytic: [10, 3]."""
    EEt = E @ E.T
    cof = np.array([[E[(i + 1) % 3, (j + 1) % 3] * E[(i + 2) % 3, (j + 2) % 3] - E[(i + 1) % 3, (j + 2) % 3] * E[(i + 2) % 3, (j + 1) % 3]
                     for j in range(3)] for i in range(3)])
    cols = []
    for D in basis[:3]:
        d9 = 2 * (D @ E.T @ E + E @ D.T @ E + EEt @ D) - 2 * np.trace(E @ D.T) * E - np.trace(EEt) * D
        cols.append(np.concatenate([d9.reshape(9), [(cof * D).sum()]]))
    return np.stack(cols, 1)


def five_point(x0, x1):
    """x0, x1 [5, 2] calibrated -> (list of unit-norm E [3, 3] with x1^T E x0 = 0, kept by the kernel's rule: every constraint
    <= 1e-9 at unit Frobenius norm; near_double).  near_double: two eigenvalues of the action matrix lie within 1e-6 (relative) of
    each other, where the number of real solutions is a matter of rounding (the convention of geometry_ref.seven_point).  The
    solutions come in the order of the eigenvalues in THIS null-space basis, which is not the kernel's."""
    x0, x1 = np.asarray(x0, dtype=np.float64), np.asarray(x1, dtype=np.float64)
    u0, v0, u1, v1 = x0[:, 0], x0[:, 1], x1[:, 0], x1[:, 1]
    A = np.stack([u1 * u0, u1 * v0, u1, v1 * u0, v1 * v0, v1, u0, v0, np.ones(5)], 1)
    if not np.isfinite(A).all():
        return [], False
    basis = np.linalg.svd(A)[2][5:9].reshape(4, 3, 3)                  # X Y Z W
    # entries of E as linear polynomials in (x, y, z)
    lin = np.zeros((3, 3, 2, 2, 2))
    lin[:, :, 1, 0, 0], lin[:, :, 0, 1, 0], lin[:, :, 0, 0, 1], lin[:, :, 0, 0, 0] = basis
    mul = _pmul3
    EEt = [[sum(mul(lin[i, k], lin[j, k]) for k in range(3)) for j in range(3)] for i in range(3)]
    tr = EEt[0][0] + EEt[1][1] + EEt[2][2]
    polys = [2 * sum(mul(EEt[i][k], lin[k, j]) for k in range(3)) - mul(tr, lin[i, j]) for i in range(3) for j in range(3)]
    polys.append(mul(mul(lin[1, 1], lin[2, 2]) - mul(lin[1, 2], lin[2, 1]), lin[0, 0])
                 - mul(mul(lin[1, 0], lin[2, 2]) - mul(lin[1, 2], lin[2, 0]), lin[0, 1])
                 + mul(mul(lin[1, 0], lin[2, 1]) - mul(lin[1, 1], lin[2, 0]), lin[0, 2]))
    Mx = np.array([[p[m] for m in _DEG3 + _BASIS] for p in polys])
    try:
        Bm = np.linalg.solve(Mx[:, :10], Mx[:, 10:])                    # degree-3 monomial i = -Bm[i] . basis monomials
    except np.linalg.LinAlgError:
        return [], False
    if not np.isfinite(Bm).all():
        return [], False
    Ax = np.zeros((10, 10))                                             # Ax b = x b at a solution, b the basis monomials there
    Ax[:6] = -Bm[:6]
    Ax[6, 0] = Ax[7, 1] = Ax[8, 2] = Ax[9, 6] = 1.0
    lam, vec = np.linalg.eig(Ax)
    near = any(abs(lam[i] - lam[j]) <= 1e-6 * max(1.0, abs(lam[i])) for i in range(10) for j in range(i))
    out = []
    for k in np.argsort(lam.real, kind="stable"):
        if abs(lam[k].imag) > 1e-9 * max(1.0, abs(lam[k])) or not abs(vec[9, k]) > 0:
            continue
        p = (vec[6:9, k] / vec[9, k]).real
        if not np.isfinite(p).all():
            continue
        build = lambda q: q[0] * basis[0] + q[1] * basis[1] + q[2] * basis[2] + basis[3]
        f = np.linalg.norm(essential_constraints(build(p)))
        for _ in range(3):                                              # Gauss-Newton on the ten constraints, kept if it lowers them
            E = build(p)
            J = _constraint_jacobian(E, basis)
            step = np.linalg.lstsq(J, -essential_constraints(E), rcond=None)[0]
            fn = np.linalg.norm(essential_constraints(build(p + step)))
            if not fn < f:
                break
            p, f = p + step, fn
        E = build(p)
        nrm = np.linalg.norm(E)
        if not (nrm > 0 and np.isfinite(nrm)):
            continue
        E = E / nrm
        if np.abs(essential_constraints(E)).max() <= 1e-9:
            out.append(E)
    return out, bool(near)


def decompose_essential(E):
    """kornia 0.6 decompose_essential_matrix + motion_from_essential: the four (R, t) in kornia's order (R1, t), (R1, -t), (R2, t),
    (R2, -t), with R1 = U W V^T, R2 = U W^T V^T, t = U[:, 2], the last column of U / row of V^T flipped when the determinant is
    negative.  The SVD's signs are free (flipping u0 and v0 together swaps R1 with R2 and t with -t), so the ORDER of the four is
    comparable with the kernel's only as a set; it matters only when two candidates tie in the depth count."""
    U, _, Vt = np.linalg.svd(E)
    if np.linalg.det(U) < 0:
        U[:, 2] = -U[:, 2]
    if np.linalg.det(Vt) < 0:
        Vt[2] = -Vt[2]
    Wm = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    R1, R2, t = U @ Wm @ Vt, U @ Wm.T @ Vt, U[:, 2]
    return [(R1, t), (R1, -t), (R2, t), (R2, -t)]


def positive_depths(R, t, x0, x1):
    """Number of correspondences in front of both cameras by the linear two-view depth: d0 least squares in x1 x (d0 R x0 + t) = 0."""
    h0 = np.concatenate([x0, np.ones((len(x0), 1))], 1)
    h1 = np.concatenate([x1, np.ones((len(x1), 1))], 1)
    r = h0 @ R.T
    a, b = np.cross(h1, r), np.cross(h1, np.broadcast_to(t, h1.shape))
    with np.errstate(divide="ignore", invalid="ignore"):
        d0 = -(a * b).sum(1) / (a * a).sum(1)
    d1 = d0 * r[:, 2] + t[2]
    return int(((d0 > 0) & (d1 > 0)).sum())


def relative_pose(k0, k1, m0, K0, K1, R, T, nk=None, threshold=1.0, hypotheses=1000, seed=0, pair=0):
    """og_relative_pose for one pair, in float64: the validity rule, (x - c) / f, the fp32 threshold of ransac_threshold, the
    kernel's draws (geometry_ref.draw_distinct, k = 5), five_point, squared Sampson error <= thr^2 counted over the valid matches,
    most inliers winning and then the lowest (hypothesis, solution), kornia's four (R, t), the depth count with the first maximum,
    pose_error against (R, T).  -> {'E', 'R', 't', 'inliers' [M] bool, 'num_inliers', 'error' (inf without a model), 'hypothesis'
    (-1 without a model), 'ransac_inliers'}.  The solutions of one hypothesis are ordered in five_point's basis, not the kernel's, so
    only the hypothesis part of the winner is comparable; and the kernel scores in fp32, so counts may differ by the matches that lie
    on the threshold to rounding."""
    from tests import geometry_ref
    M = len(np.asarray(m0))
    K0n, K1n = np.asarray(K0, dtype=np.float64), np.asarray(K1, dtype=np.float64)
    idx, p0, p1 = geometry_ref.valid_matches(np.asarray(k0), np.asarray(k1), np.asarray(m0), nk)
    none = {"E": np.zeros((3, 3)), "R": np.zeros((3, 3)), "t": np.zeros(3), "inliers": np.zeros(M, dtype=bool), "num_inliers": 0,
            "error": math.inf, "hypothesis": -1, "ransac_inliers": 0}
    n = len(idx)
    if n < 5:
        return none
    x0 = (p0 - K0n[:2, 2]) / K0n[[0, 1], [0, 1]]
    x1 = (p1 - K1n[:2, 2]) / K1n[[0, 1], [0, 1]]
    thr = ransac_threshold(threshold, torch.as_tensor(K0n), torch.as_tensor(K1n))
    t2 = float(np.float32(thr) * np.float32(thr))
    best, best_E, best_h = -1, None, -1
    for h in range(hypotheses):
        pick = geometry_ref.draw_distinct(seed, pair, h, n, k=5)
        for E in five_point(x0[pick], x1[pick])[0]:
            cnt = int((geometry_ref.sampson_sq(E, x0, x1) <= t2).sum())
            if cnt > best:
                best, best_E, best_h = cnt, E, h
    if best_E is None:
        return none
    inl = geometry_ref.sampson_sq(best_E, x0, x1) <= t2
    cands = decompose_essential(best_E)
    counts = [positive_depths(Rc, tc, x0[inl], x1[inl]) for Rc, tc in cands]
    Rb, tb = cands[int(np.argmax(counts))]
    mask = np.zeros(M, dtype=bool)
    mask[idx[inl]] = True
    err = pose_error(torch.as_tensor(np.asarray(R, dtype=np.float64)), torch.as_tensor(np.asarray(T, dtype=np.float64)),
                     torch.from_numpy(Rb.copy()), torch.from_numpy(tb.copy()))
    return {"E": best_E, "R": Rb, "t": tb, "inliers": mask, "num_inliers": int(inl.sum()), "error": err, "hypothesis": best_h,
            "ransac_inliers": best}
