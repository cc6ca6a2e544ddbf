"""Crafted inputs for the stages of csrc/metrics.hip: minimal five-point problems by family, two-view scenes for og_relative_pose and
the boundary cases of og_epipolar_precision.  No kernel is launched from here; tests/test_metrics_cases_cpu.py proves that every case
reaches the edge it names, tests/test_gpu_metrics_stages.py runs them on the GPU against tests/metrics_ref.py."""
import functools
import math

import numpy as np
import torch

from tests import geometry_ref, metrics_ref

# ------------------------------------------------------------------------------------------------ minimal problems
P = 64                               # problems per family
FAMILIES = ("generic", "forward", "forward_near", "forward_no_rotation", "roll", "translation", "rot120", "planar", "forward_f32")
DEGENERATE = ("duplicate", "rotation_only", "rectified")


def rot(axis, deg):
    ax = np.asarray(axis, dtype=np.float64)
    ax = ax / np.linalg.norm(ax)
    Kx = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    a = math.radians(deg)
    return np.eye(3) + math.sin(a) * Kx + (1 - math.cos(a)) * Kx @ Kx


def _unit(v):
    return v / np.linalg.norm(v)


def _pose(family, rng, p):
    """(R, T) of problem p of a family."""
    any_R = lambda: rot(rng.standard_normal(3), 30.0 * rng.random())
    any_T = lambda: _unit(rng.standard_normal(3))
    sign = 1.0 if p % 2 == 0 else -1.0
    if family in ("generic", "planar", "duplicate"):
        return any_R(), any_T()
    if family in ("forward", "forward_f32"):
        return any_R(), np.array([0.0, 0.0, sign])
    if family == "forward_near":                     # the first half 1e-3 degrees off the axis, the second half 0.1 degrees
        off = math.radians(1e-3 if p < P // 2 else 0.1)
        az = 2 * math.pi * rng.random()
        return any_R(), sign * np.array([math.sin(off) * math.cos(az), math.sin(off) * math.sin(az), math.cos(off)])
    if family == "forward_no_rotation":
        return np.eye(3), np.array([0.0, 0.0, sign])
    if family == "roll":
        return rot([0.0, 0.0, 1.0], sign * (5.0 + 170.0 * rng.random())), any_T()
    if family == "translation":
        return np.eye(3), any_T()
    if family == "rot120":
        return rot(rng.standard_normal(3), 120.0), any_T()
    if family == "rotation_only":
        return any_R(), np.zeros(3)
    if family == "rectified":
        return np.eye(3), np.array([1.0, 0.0, 0.0])
    raise KeyError(family)


def minimal_problems(family, seed=0):
    """-> {'x0' [P, 5, 2], 'x1' [P, 5, 2] float64, 'E' [P, 3, 3] the true essential matrix at unit norm (zeros where T = 0), 'E_scene'
    [T]x R of the pose at unit norm, 'R' [P, 3, 3], 'T' [P, 3]}.  Points of image 0 in [-0.5, 0.5]^2 at depth 3-8, image 1 their exact
    projection (|depth in camera 1| > 0.5).  'E' is 'E_scene' except for forward_f32: the rounded points are not on the scene's
    epipolar lines, so the problem's own solution next to E_scene (refine_truth) is the truth there."""
    rng = np.random.default_rng([seed, (FAMILIES + DEGENERATE).index(family)])
    x0, x1, Es, Rs, Ts = (np.zeros((P, 5, 2)), np.zeros((P, 5, 2)), np.zeros((P, 3, 3)), np.zeros((P, 3, 3)), np.zeros((P, 3)))
    for p in range(P):
        R, T = _pose(family, rng, p)
        if family == "planar":                       # a plane n . X = 5 tilted up to 30 degrees against the image plane
            n = rot(rng.standard_normal(3) * [1, 1, 0] + [0, 0, 1e-9], 30.0 * rng.random()) @ np.array([0.0, 0.0, 1.0])
        k = 0
        while k < 5:
            u = rng.random(2) - 0.5
            ray = np.array([u[0], u[1], 1.0])
            z = 5.0 / (n @ ray) if family == "planar" else 3.0 + 5.0 * rng.random()
            Y = R @ (ray * z) + T
            if abs(Y[2]) > 0.5 and 3.0 <= z <= 8.0:
                x0[p, k], x1[p, k] = u, Y[:2] / Y[2]
                k += 1
        if family == "duplicate":
            x0[p, 1], x1[p, 1] = x0[p, 0], x1[p, 0]
        E = np.array([[0, -T[2], T[1]], [T[2], 0, -T[0]], [-T[1], T[0], 0]]) @ R
        Es[p] = E / np.linalg.norm(E) if np.linalg.norm(E) > 0 else E
        Rs[p], Ts[p] = R, T
    E_scene = Es.copy()
    if family == "forward_f32":
        x0, x1 = x0.astype(np.float32).astype(np.float64), x1.astype(np.float32).astype(np.float64)
        Es = np.stack([refine_truth(Es[p], x0[p], x1[p]) for p in range(P)])
    return {"x0": x0, "x1": x1, "E": Es, "E_scene": E_scene, "R": Rs, "T": Ts}


def refine_truth(E, x0, x1):
    """Newton from E onto the solution set of the minimal problem (x0, x1): the five epipolar equations, the ten constraints and unit
    norm, 16 equations in the 9 entries, least squares with a central-difference Jacobian.  Independent of both solvers: no null
    space, no elimination, no eigenproblem.  With exact points E is already a solution; with points rounded to fp32 the solution moves
    by the rounding (2^-25 relative) times the problem's condition number, 1e-7 to 1e-5 here, more than either solver's own error."""
    u0, v0, u1, v1 = x0[:, 0], x0[:, 1], x1[:, 0], x1[:, 1]
    A = np.stack([u1 * u0, u1 * v0, u1, v1 * u0, v1 * v0, v1, u0, v0, np.ones(5)], 1)
    res = lambda e: np.concatenate([A @ e, metrics_ref.essential_constraints(e.reshape(3, 3)), [e @ e - 1.0]])
    e = E.reshape(9).copy()
    for _ in range(6):
        J = np.stack([(res(e + 1e-6 * d) - res(e - 1e-6 * d)) / 2e-6 for d in np.eye(9)], 1)
        e = e + np.linalg.lstsq(J, -res(e), rcond=None)[0]
    return (e / np.linalg.norm(e)).reshape(3, 3)


@functools.lru_cache(maxsize=None)
def solved(family):
    """(minimal_problems(family), the restatement's (solutions, near_double) of each problem).  Computed once per process."""
    m = minimal_problems(family)
    return m, [metrics_ref.five_point(m["x0"][p], m["x1"][p]) for p in range(P)]


def error_of_true(sols, Et):
    """max-abs distance of the nearest solution to the true E, up to sign (inf without a solution)."""
    return min([min(np.abs(s - Et).max(), np.abs(s + Et).max()) for s in sols] or [np.inf])


# ------------------------------------------------------------------------------------------------ scenes for relative_pose
def pose_scene(n, R=None, T=None, outliers=0.0, noise=0.0, seed=0, thr_px=1.0, Ks=None):
    """geometry_ref.make_scene for one pair with the pose given: (k0 [1, n, 2], k1 [1, n, 2] fp32, matches0 [1, n], truth, outlier
    mask [1, n]).  R, T: numpy [3, 3] / [3], None for make_scene's own random pose (then this IS make_scene).  Ks: the two intrinsics
    (float64 [3, 3]) instead of drawn ones."""
    if R is None and T is None:
        return geometry_ref.make_scene(1, n, outliers=outliers, noise=noise, seed=seed, thr_px=thr_px)
    g = torch.Generator().manual_seed(seed)
    drawn = []
    for _ in range(2):
        f = 400 + 800 * float(torch.rand(1, generator=g))
        drawn.append(torch.tensor([[f * (0.95 + 0.1 * float(torch.rand(1, generator=g))), 0, geometry_ref.W / 2 + 20 * float(torch.randn(1, generator=g))],
                                   [0, f, geometry_ref.H / 2 + 20 * float(torch.randn(1, generator=g))], [0, 0, 1]], dtype=torch.float64))
    Ks = drawn if Ks is None else Ks
    R = torch.from_numpy(np.asarray(R, dtype=np.float64)) if R is not None else geometry_ref._rot(g, 30.0)
    T = torch.from_numpy(np.asarray(T, dtype=np.float64))
    wh = torch.tensor([geometry_ref.W - 1.0, geometry_ref.H - 1.0])
    pts = []
    while sum(p.shape[0] for p in pts) < n:
        px = torch.rand(4 * n, 2, generator=g, dtype=torch.float64) * wh
        z = 3 + 5 * torch.rand(4 * n, 1, generator=g, dtype=torch.float64)
        X = torch.cat([(px - Ks[0][:2, 2]) / Ks[0][[0, 1], [0, 1]], torch.ones_like(z)], 1) * z
        Y = X @ R.T + T
        p1 = Y[:, :2] / Y[:, 2:] * Ks[1][[0, 1], [0, 1]] + Ks[1][:2, 2]
        keep = (Y[:, 2] > 0.5) & (p1 >= 0).all(1) & (p1 <= wh).all(1)          # a 90 degree roll takes much of image 0 out of image 1
        pts.append(torch.cat([px, p1], 1)[keep])
    Pm = torch.cat(pts)[:n]
    p0, p1 = Pm[:, :2].clone(), Pm[:, 2:].clone()
    if noise:
        p0 += noise * torch.randn(n, 2, generator=g, dtype=torch.float64)
        p1 += noise * torch.randn(n, 2, generator=g, dtype=torch.float64)
    E = metrics_ref.essential_from_Rt(R, T)
    out_mask = torch.zeros(1, n, dtype=torch.bool)
    n_out = int(round(outliers * n))
    if n_out:
        thr = metrics_ref.ransac_threshold(thr_px, Ks[0], Ks[1])
        idx = torch.randperm(n, generator=g)[:n_out]
        x0o = metrics_ref.normalize_with_intrinsics(p0[idx], Ks[0])
        todo = torch.ones(n_out, dtype=torch.bool)
        for _ in range(100):
            c = torch.rand(n_out, 2, generator=g, dtype=torch.float64) * wh
            ok = todo & (metrics_ref.sampson_error(x0o, metrics_ref.normalize_with_intrinsics(c, Ks[1]), E) > (geometry_ref.OUT_SEP * thr) ** 2)
            p1[idx[ok]] = c[ok]
            todo &= ~ok
        out_mask[0, idx[~todo]] = True
    tr = {"K0": Ks[0][None], "K1": Ks[1][None], "R": R[None], "T": T[None]}
    return p0.float()[None], p1.float()[None], torch.arange(n)[None], tr, out_mask


def with_holes(scene, M, seed):
    """Spread a scene's n matches over M > n rows of keypoints0 (the other rows unmatched, at random pixels) and permute keypoints1,
    so that a match's compacted position, its row and its partner's index all differ.  -> (k0 [1, M, 2], k1, matches0 [1, M], truth,
    outlier mask [1, M] (False on the holes), rows [n] of the matches)."""
    k0, k1, _, tr, out = scene
    n = k0.shape[1]
    g = torch.Generator().manual_seed(seed)
    rows = torch.sort(torch.randperm(M, generator=g)[:n]).values
    K0 = torch.rand(1, M, 2, generator=g) * torch.tensor([geometry_ref.W - 1.0, geometry_ref.H - 1.0])
    K0[0, rows] = k0[0]
    perm = torch.randperm(n, generator=g)
    m0 = torch.full((1, M), -1, dtype=torch.int64)
    m0[0, rows] = torch.argsort(perm)
    O = torch.zeros(1, M, dtype=torch.bool)
    O[0, rows] = out[0]
    return K0, k1[:, perm], m0, tr, O, rows


CHUNK_SCENES = {"chunk-1025": (1025, 1200), "chunk-1100": (1100, 1300), "chunk-2049": (2049, 2300)}     # name -> (valid matches, M)


def chunk_scene(name):
    n, M = CHUNK_SCENES[name]
    return with_holes(geometry_ref.make_scene(1, n, outliers=0.3, seed=100 + n), M, seed=200 + n)


def two_motion_scene():
    """'chunk-two-motions': 2049 valid matches among M = 2300 rows.  The first 1024 in index order (the scorer's first staging pass)
    follow pose A (about 70 %) or nothing, and every one of them lies more than OUT_SEP thresholds from pose B's geometry; the other
    1025 all follow pose B, which is the truth handed to the kernel.  Over all matches B holds 1025 and A about 700, so B wins; a
    scorer that staged the first pass again in place of the later ones would count about 1400 for A and none for B.
    -> (k0, k1, matches0, truth of B, outlier mask (True on the first part), rows, truth of A)."""
    b = geometry_ref.make_scene(1, 1025, seed=121)
    trB = b[3]
    Ks = [trB["K0"][0], trB["K1"][0]]
    g = torch.Generator().manual_seed(122)
    T = torch.randn(3, generator=g, dtype=torch.float64)
    a = pose_scene(1600, R=geometry_ref._rot(g, 30.0).numpy(), T=(T / T.norm()).numpy(), outliers=0.3, seed=123, Ks=Ks)
    x0 = metrics_ref.normalize_with_intrinsics(a[0][0], Ks[0])
    x1 = metrics_ref.normalize_with_intrinsics(a[1][0], Ks[1])
    thr = metrics_ref.ransac_threshold(1.0, Ks[0], Ks[1])
    far = metrics_ref.sampson_error(x0, x1, metrics_ref.essential_from_Rt(trB["R"][0], trB["T"][0])) > (geometry_ref.OUT_SEP * thr) ** 2
    keep = torch.nonzero(far)[:1024, 0]
    assert len(keep) == 1024
    k0 = torch.cat([a[0][:, keep], b[0]], 1)
    k1 = torch.cat([a[1][:, keep], b[1]], 1)
    out = torch.cat([torch.ones(1, 1024, dtype=torch.bool), torch.zeros(1, 1025, dtype=torch.bool)], 1)
    K0, K1, m0, _, O, rows = with_holes((k0, k1, None, trB, out), 2300, seed=124)
    trA = {**trB, "R": a[3]["R"], "T": a[3]["T"]}
    return K0, K1, m0, trB, O, rows, trA


def forward_scene():
    g = torch.Generator().manual_seed(300)
    return pose_scene(300, R=geometry_ref._rot(g, 30.0).numpy(), T=[0.0, 0.0, 1.0], outliers=0.3, seed=301)


def roll_scene():
    g = torch.Generator().manual_seed(310)
    T = torch.randn(3, generator=g, dtype=torch.float64)
    return pose_scene(300, R=rot([0.0, 0.0, 1.0], 90.0), T=(T / T.norm()).numpy(), outliers=0.3, seed=311)


def clean_flags(m0, out, nk=None):
    """The truth (True = inlier) over a pair's valid matches in index order, for seed_with_clean_samples."""
    m0, out = np.asarray(m0), np.asarray(out)
    lim = len(m0) if nk is None else min(int(nk), len(m0))
    return [not bool(out[i]) for i in range(lim) if m0[i] >= 0]


def draws_clean_sample(clean, seed, hypotheses, pair=0):
    """Whether one of the pair's `hypotheses` draws under `seed` picks five matches that are all flagged in `clean`."""
    return any(all(clean[r] for r in geometry_ref.draw_distinct(seed, pair, h, len(clean), k=5)) for h in range(hypotheses))


def seed_with_clean_samples(clean, hypotheses, pair_offset=0):
    """tests/test_gpu_geometry.py's rule for five draws: the first seed under which every pair draws an all-inlier sample."""
    for seed in range(200):
        if all(any(all(c[r] for r in geometry_ref.draw_distinct(seed, pair_offset + b, h, len(c), k=5)) for h in range(hypotheses))
               for b, c in enumerate(clean)):
            return seed
    raise AssertionError("no seed below 200 draws a clean sample for every pair")


# error-formula: (alpha, beta, s) -> the truth handed to the kernel is R' = R Rot(axis, alpha), T' = s Rot(axis2, beta) T
ERROR_FORMULA = [(0.0, 0.0, 1.0), (45.0, 1.0, 1.0), (1.0, 60.0, 5.0), (2.0, 120.0, 0.2), (0.0, 180.0, 1.0), (179.0, 0.0, 1.0), (3.0, 90.0, 1.0)]


def error_formula_truths():
    """-> (scene of 64 noise-free matches without outliers, [(truth dict, expected error max(alpha, min(beta, 180 - beta)))])."""
    scene = geometry_ref.make_scene(1, 64, seed=400)
    tr = scene[3]
    R, T = tr["R"][0].numpy(), tr["T"][0].numpy()
    rng = np.random.default_rng(401)
    perp = _unit(np.cross(T, rng.standard_normal(3)))          # rotating T about an axis perpendicular to it turns it by exactly beta
    out = []
    for alpha, beta, s in ERROR_FORMULA:
        R2 = R @ rot(rng.standard_normal(3), alpha)
        T2 = s * (rot(perp, beta) @ T)
        out.append(({**tr, "R": torch.from_numpy(R2)[None], "T": torch.from_numpy(T2)[None]}, max(alpha, min(beta, 180.0 - beta))))
    return scene, out


EDGE_PAIRS = ("none", "four", "five", "chance", "holes", "entry_N", "entries_1000", "nk_cuts", "nk_large", "one_spot")


def edges():
    """One batch, M = 70, N = 64 -> (k0, k1, matches0, truth, nk [B] int32, info).  Pair names in EDGE_PAIRS order.  info['entry_N_row']:
    the row of pair 'entry_N' whose entry is == N; keypoints1[b + 1][0], which an unchecked read at index N of pair b would fetch, is
    placed where that row's true partner lies, so the row would count as an inlier."""
    M, N, B = 70, 64, len(EDGE_PAIRS)
    k0, k1, _, tr, _ = geometry_ref.make_scene(B, M, seed=500)
    full = k1.clone()
    k1 = k1[:, :N].clone()
    g = torch.Generator().manual_seed(501)
    m0 = torch.arange(M).repeat(B, 1)
    m0[m0 >= N] = -1
    b = EDGE_PAIRS.index
    m0[b("none")] = -1
    m0[b("four"), 4:] = -1
    m0[b("five"), :20] = -1
    m0[b("five"), 25:] = -1
    k0[b("chance")] = torch.rand(M, 2, generator=g) * torch.tensor([639.0, 479.0])
    m0[b("chance"), 12:] = -1
    m0[b("holes")][torch.rand(M, generator=g) < 0.3] = -1
    # entry == N: the kernel's row N of this pair is row 0 of the next pair.  The next pair ('entries_1000') gets, as its keypoint 0,
    # the true partner of row 64 of this pair under THIS pair's pose, and its own row 0 unmatched.
    e = b("entry_N")
    assert e + 1 < B
    m0[e, N] = N
    k1[e + 1, 0] = full[e, N]                      # make_scene's keypoints1 row N is the exact partner of keypoints0 row N
    m0[e + 1, 0] = -1
    m0[e + 1, N:] = 1000
    m0[b("nk_cuts")] = torch.arange(M)
    m0[b("nk_cuts")][m0[b("nk_cuts")] >= N] = -1
    m0[b("nk_large"), 40:] = -1
    k0[b("one_spot")], k1[b("one_spot")] = torch.tensor([100.0, 120.0]), torch.tensor([50.0, 60.0])
    nk = torch.full((B,), M, dtype=torch.int32)
    nk[b("nk_cuts")] = 30
    nk[b("nk_large")] = 1000
    return k0, k1, m0, tr, nk, {"entry_N_row": N, "M": M, "N": N}


HYPOTHESIS_COUNTS = (1, 25, 26, 128)               # 10, 250, 260 (a second group of 4 live lanes) and 1280 = 5 x 256 models


# ------------------------------------------------------------------------------------------------ epipolar precision
def precision_truth(B):
    eye = torch.eye(3, dtype=torch.float64)
    return {"K0": eye.repeat(B, 1, 1), "K1": eye.repeat(B, 1, 1), "R": eye.repeat(B, 1, 1), "T": torch.tensor([[1.0, 0.0, 0.0]], dtype=torch.float64).repeat(B, 1)}


def precision_boundary(k):
    """K = I, R = I, T = (1, 0, 0): d = 2 (v0 - v1)^2 exactly.  One pair of M = 257 rows; row i has v0 - v1 = 2^-k for i % 3 == 0 and
    0 otherwise, u0, u1 arbitrary dyadic numbers; rows 250.. are unmatched.  -> (k0, k1, m0, truth, d = 2^(1 - 2k), rows at the boundary)."""
    M = 257
    i = torch.arange(M, dtype=torch.float64)
    v1 = (i % 16) / 16.0
    off = torch.where(torch.arange(M) % 3 == 0, 2.0 ** -k, 0.0).double()
    k0 = torch.stack([(i % 7) / 8.0, v1 + off], 1)
    k1 = torch.stack([(i % 5) / 4.0 + 0.25, v1], 1)
    m0 = torch.arange(M)
    m0[250:] = -1
    assert torch.equal(k0.float().double(), k0) and torch.equal(k1.float().double(), k1)
    return k0.float()[None], k1.float()[None], m0[None], precision_truth(1), 2.0 ** (1 - 2 * k), int((torch.arange(250) % 3 == 0).sum())


def precision_edges():
    """A batch with N = 8, M = 12, threshold 5e-4 -> (k0, k1, m0, truth, nk, expected (num_correct, precision, matching_score) per pair).
    Pairs: 0 nk < M cuts a correct match off; 1 nk > M; 2 entries == N and beyond; 3 precision and matching score differ; 4 no match."""
    B, M, N = 5, 12, 8
    k1 = torch.zeros(B, N, 2)
    k1[:, :, 0] = torch.arange(N) / 8.0
    k1[:, :, 1] = torch.arange(N) / 4.0
    k0 = torch.zeros(B, M, 2)
    m0 = torch.full((B, M), -1, dtype=torch.int64)
    far = 0.5                                       # d = 0.5: not correct
    def put(b, i, j, good):
        m0[b, i] = j
        k0[b, i, 0] = 0.125 * i
        k0[b, i, 1] = k1[b, j, 1] + (0.0 if good else far)
    for i in range(6):
        put(0, i, i, i in (0, 5))                   # correct: rows 0 and 5; nk = 5 cuts row 5
    for i in range(6):
        put(1, i, 7 - i, i % 2 == 0)                # 3 of 6, nk = 100 > M
    for i in range(4):
        put(2, i, i, True)
    m0[2, 4], m0[2, 5], m0[2, 6] = N, N + 1, 1000   # not matches; their keypoints lie on a partner's line
    k0[2, 4:7, 1] = k1[2, 0, 1]
    for i in range(4):
        put(3, i, i, i < 3)                         # 3 of 4 matched, 12 detected: precision 0.75, matching score 0.25
    nk = torch.tensor([5, 100, M, M, M], dtype=torch.int32)
    expect = [(1, 1 / 5, 1 / 5), (3, 3 / 6, 3 / 12), (4, 1.0, 4 / 12), (3, 3 / 4, 3 / 12), (0, 0.0, 0.0)]
    return k0, k1, m0, precision_truth(B), nk, expect
