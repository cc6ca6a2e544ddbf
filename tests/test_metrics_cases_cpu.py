"""The crafted cases of tests/metrics_cases.py reach the edges they name, and the float64 restatement they are judged by
(tests/metrics_ref.py: five_point, relative_pose) is sound on them.  No kernel is launched; the last test runs the solver text of
csrc/metrics.hip on the host (tests/host/five_point_host.cpp) through every family.

Measured on the CPU: the restatement finds the true E of all 9 x 64 non-degenerate problems, worst error 5e-13, none near-double.
With the points rounded to fp32 (forward_f32) the essential matrix of the unrounded scene lies 2e-7 (median) to 6e-6 from the
problem's own solution, so there the truth is that solution (metrics_cases.refine_truth), which the restatement finds to 4e-13.
The host path of the kernel's solver, all 12 x 64 problems: every non-degenerate one within the rule e <= max(10 e_ref, 1e-9) and
with the restatement's count; before the reflection 0 of 64 forward problems, and with the reflection and three polish steps
63 of 64 forward_near ones (see csrc/metrics.hip: kPolishSteps)."""
import math
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from tests import geometry_ref, metrics_cases as mc, metrics_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


solved = mc.solved


def valid(sols, x0, x1):
    h0, h1 = np.c_[x0, np.ones(5)], np.c_[x1, np.ones(5)]
    return all(abs(np.linalg.norm(E) - 1) < 1e-9 and np.abs(ref.essential_constraints(E)).max() <= 1e-9
               and np.abs(np.einsum("ni,ij,nj->n", h1, E, h0)).max() <= 1e-9 for E in sols)


# ------------------------------------------------------------------------------------------------ minimal problems
@pytest.mark.parametrize("family", mc.FAMILIES)
def test_restatement_finds_the_true_E(family):
    m, sols = solved(family)
    near = 0
    for p in range(mc.P):
        s, nd = sols[p]
        near += nd
        assert valid(s, m["x0"][p], m["x1"][p]) and len(s) <= 10, p
        assert mc.error_of_true(s, m["E"][p]) <= 1e-7, (p, mc.error_of_true(s, m["E"][p]))
        assert all(mc.error_of_true([s[i]], s[j]) > 1e-6 for i in range(len(s)) for j in range(i)), p
    assert near <= 0.01 * mc.P, near


@pytest.mark.parametrize("family", mc.FAMILIES)
def test_family_has_its_structure(family):
    m, _ = solved(family)
    x0, x1, E = m["x0"], m["x1"], m["E_scene"]
    assert np.abs(x0).max() <= 0.5 and np.isfinite(x1).all()
    assert np.allclose(np.linalg.norm(E.reshape(mc.P, 9), axis=1), 1.0, atol=1e-12)
    if family in ("forward", "forward_no_rotation", "forward_f32"):
        assert not E[:, 2].any()                                  # the third row of [T]x R is zero: the old chart's point at infinity
        assert set(m["T"][:, 2]) == {1.0, -1.0}
    if family == "forward_near":
        row = np.linalg.norm(E[:, 2], axis=1)
        assert (row > 0).all() and row[:mc.P // 2].max() <= math.sin(math.radians(1e-3)) and row.max() <= math.sin(math.radians(0.1))
        assert row[mc.P // 2:].min() > math.sin(math.radians(1e-3))
    if family in ("roll", "translation"):
        assert not E[:, 2, 2].any()                               # E[2][2] = 0: the old chart's coefficient of W
    if family == "forward_no_rotation":
        d = x1[:, :, 0] * x0[:, :, 1] - x1[:, :, 1] * x0[:, :, 0]     # u1 v0 == v1 u0: columns 1 and 3 of the constraints coincide
        assert np.abs(d).max() <= 4 * np.finfo(np.float64).eps
    if family == "roll":
        ang = np.degrees(np.arccos(np.clip((np.trace(m["R"], axis1=1, axis2=2) - 1) / 2, -1, 1)))
        assert ang.min() >= 5.0 and ang.max() <= 175.0 and np.abs(m["R"][:, 2, 2] - 1).max() < 1e-15
    if family == "rot120":
        assert np.allclose(np.trace(m["R"], axis1=1, axis2=2), 0.0, atol=1e-12)       # 1 + 2 cos 120 = 0
    if family == "planar":
        for p in range(mc.P):                                      # the five points of image 0, lifted by their depths, span a plane
            _, s = solved_depth_plane(x0[p], x1[p], m["R"][p], m["T"][p])
            assert s < 1e-12, (p, s)
    if family == "forward_f32":
        assert np.array_equal(x0.astype(np.float32).astype(np.float64), x0) and np.array_equal(x1.astype(np.float32).astype(np.float64), x1)
        moved = np.abs(m["E"] - m["E_scene"]).reshape(mc.P, 9).max(1)
        # the rounding (2^-25 relative, points of order 0.5) times a condition number of up to ~1e4: the same root, not another one
        assert 0 < moved.max() <= 1e-3, moved.max()
        for p in range(mc.P):
            assert valid([m["E"][p]], x0[p], x1[p]), p             # the refined truth solves the rounded problem


def solved_depth_plane(x0, x1, R, T):
    """Depths of the five points from the pose, and the smallest singular value of [X 1] (zero when the points are coplanar)."""
    h0, h1 = np.c_[x0, np.ones(5)], np.c_[x1, np.ones(5)]
    a, b = np.cross(h1, h0 @ R.T), np.cross(h1, np.broadcast_to(T, (5, 3)))
    z = -(a * b).sum(1) / (a * a).sum(1)
    X = h0 * z[:, None]
    sv = np.linalg.svd(np.c_[X, np.ones(5)] / 8.0, compute_uv=False)
    return z, sv[3]


@pytest.mark.parametrize("family", mc.DEGENERATE)
def test_degenerate_group_is_degenerate(family):
    m, sols = solved(family)
    x0, x1 = m["x0"], m["x1"]
    if family == "duplicate":
        assert np.array_equal(x0[:, 0], x0[:, 1]) and np.array_equal(x1[:, 0], x1[:, 1])
    if family == "rotation_only":
        assert not m["T"].any() and not m["E"].any()
    if family == "rectified":
        assert np.abs(x0[:, :, 1] - x1[:, :, 1]).max() <= 1e-15    # every match on its scanline
    for p in range(mc.P):
        s, _ = sols[p]
        assert 0 <= len(s) <= 10 and all(np.isfinite(E).all() for E in s) and valid(s, x0[p], x1[p]), p


# ------------------------------------------------------------------------------------------------ scenes
@pytest.mark.parametrize("name", sorted(mc.CHUNK_SCENES))
def test_chunk_scenes_cross_the_seam(name):
    n, M = mc.CHUNK_SCENES[name]
    k0, k1, m0, tr, out, rows = mc.chunk_scene(name)
    idx, _, _ = geometry_ref.valid_matches(k0[0].numpy(), k1[0].numpy(), m0[0].numpy())
    assert len(idx) == n > 1024 and M > n and k0.shape[1] == M and k1.shape[1] == n
    assert np.array_equal(idx, rows.numpy())
    # on both sides of the 1024 seam the compacted position, the row and the partner's index all differ
    for pos in (1023, 1024, n - 1):
        assert len({pos, int(idx[pos]), int(m0[0, idx[pos]])}) == 3, pos
    assert 0.25 * n <= int(out.sum()) <= 0.3 * n + 1
    # the matches that are not outliers lie on the true epipolar geometry
    x0 = ref.normalize_with_intrinsics(k0[0][idx], tr["K0"][0])
    x1 = ref.normalize_with_intrinsics(k1[0][m0[0][idx]], tr["K1"][0])
    d = ref.sampson_error(x0, x1, ref.essential_from_Rt(tr["R"][0], tr["T"][0]))
    thr = ref.ransac_threshold(1.0, tr["K0"][0], tr["K1"][0])
    good = ~out[0][idx]
    assert float(d[good].max()) < 0.01 * thr * thr and float(d[~good].min()) > (geometry_ref.OUT_SEP * thr) ** 2


def test_two_motion_scene_tells_the_staging_passes_apart():
    k0, k1, m0, trB, out, rows, trA = mc.two_motion_scene()
    idx, x0, x1 = geometry_ref.valid_matches(k0[0].numpy(), k1[0].numpy(), m0[0].numpy())
    assert len(idx) == 2049 and np.array_equal(idx, rows.numpy()) and bool(out[0][idx[:1024]].all()) and not bool(out[0][idx[1024:]].any())
    K0, K1 = trB["K0"][0].numpy(), trB["K1"][0].numpy()
    x0, x1 = (x0 - K0[:2, 2]) / K0[[0, 1], [0, 1]], (x1 - K1[:2, 2]) / K1[[0, 1], [0, 1]]
    thr = ref.ransac_threshold(1.0, trB["K0"][0], trB["K1"][0])
    dA = geometry_ref.sampson_sq(ref.essential_from_Rt(trA["R"][0], trA["T"][0]).numpy(), x0, x1)
    dB = geometry_ref.sampson_sq(ref.essential_from_Rt(trB["R"][0], trB["T"][0]).numpy(), x0, x1)
    assert dB[:1024].min() > (geometry_ref.OUT_SEP * thr) ** 2 and dB[1024:].max() < 0.01 * thr * thr
    inA, inB = dA <= thr * thr, dB <= thr * thr
    assert 650 <= inA[:1024].sum() <= 750 and inB.sum() == 1025 > inA.sum()             # scored over every match, B wins
    again = lambda f: 2 * f[:1024].sum() + f[:1].sum()                                  # the first pass staged three times over
    assert again(inA) >= 1300 and again(inB) == 0                                       # scored that way, A wins and B holds nothing


def test_forward_and_roll_scenes():
    for scene, check in ((mc.forward_scene(), lambda R, T: torch.equal(T, torch.tensor([0.0, 0.0, 1.0], dtype=torch.float64))),
                         (mc.roll_scene(), lambda R, T: abs(float(R[0, 1]) + 1) < 1e-15 and abs(float(R[2, 2]) - 1) < 1e-15)):
        k0, k1, m0, tr, out = scene
        assert k0.shape == (1, 300, 2) and check(tr["R"][0], tr["T"][0]) and 80 <= int(out.sum()) <= 90
        assert abs(float(tr["T"][0].norm()) - 1) < 1e-12 and ref.rotation_error(torch.eye(3), tr["R"][0]) <= 90.0 + 1e-9
        x0 = ref.normalize_with_intrinsics(k0[0], tr["K0"][0])
        x1 = ref.normalize_with_intrinsics(k1[0], tr["K1"][0])
        d = ref.sampson_error(x0, x1, ref.essential_from_Rt(tr["R"][0], tr["T"][0]))
        thr = ref.ransac_threshold(1.0, tr["K0"][0], tr["K1"][0])
        assert float(d[~out[0]].max()) < 0.01 * thr * thr and float(d[out[0]].min()) > (geometry_ref.OUT_SEP * thr) ** 2
        assert float(k1.min()) >= 0 and float(k1[..., 0].max()) <= geometry_ref.W and float(k1[..., 1].max()) <= geometry_ref.H


def test_error_formula_truths():
    (k0, k1, m0, tr, out), cases = mc.error_formula_truths()
    assert k0.shape == (1, 64, 2) and not bool(out.any()) and len(cases) == len(mc.ERROR_FORMULA) == 7
    want = [0.0, 45.0, 60.0, 60.0, 0.0, 179.0, 90.0]
    for (t2, expect), w, (alpha, beta, s) in zip(cases, want, mc.ERROR_FORMULA):
        assert expect == w
        # against the scene's own pose the restated formula gives the expected error; acos cannot resolve better than 1e-6 deg near 0 / 180
        assert abs(ref.pose_error(t2["R"][0], t2["T"][0], tr["R"][0], tr["T"][0]) - expect) < 2e-6
        assert abs(ref.rotation_error(t2["R"][0], tr["R"][0]) - alpha) < 2e-6
        assert abs(float(t2["T"][0].norm()) - s) < 1e-12
        c = float(t2["T"][0] @ tr["T"][0]) / s
        assert abs(math.degrees(math.acos(max(-1.0, min(1.0, c)))) - beta) < 2e-6
    # the cases tell max from min, a from min(a, 180 - a), and need T normalised
    assert any(a > min(b, 180 - b) > 0 for a, b, _ in mc.ERROR_FORMULA) and any(0 < a < min(b, 180 - b) for a, b, _ in mc.ERROR_FORMULA)
    assert any(b > 90 for _, b, _ in mc.ERROR_FORMULA) and {s for _, _, s in mc.ERROR_FORMULA} > {1.0}


def test_edges_reach_their_edges():
    k0, k1, m0, tr, nk, info = mc.edges()
    M, N = info["M"], info["N"]
    assert k0.shape == (len(mc.EDGE_PAIRS), M, 2) and k1.shape == (len(mc.EDGE_PAIRS), N, 2) and M == 70 and N == 64
    count = lambda name: len(geometry_ref.valid_matches(k0[b(name)].numpy(), k1[b(name)].numpy(), m0[b(name)].numpy(), int(nk[b(name)]))[0])
    b = mc.EDGE_PAIRS.index
    assert [count(n) for n in ("none", "four", "five", "chance")] == [0, 4, 5, 12]
    assert 5 < count("holes") < N and count("entry_N") == N and count("entries_1000") == N - 1
    assert count("nk_cuts") == 30 and int(nk[b("nk_cuts")]) < M and count("nk_large") == 40 and int(nk[b("nk_large")]) > M
    assert count("one_spot") == N and bool((k0[b("one_spot")] == k0[b("one_spot")][0]).all())
    assert int((m0[b("entries_1000")] == 1000).sum()) == M - N
    # the entry == N: not a match; the address an unchecked gather would read, keypoints1[e][N], is keypoints1[e + 1][0], inside the
    # tensor, and holds the row's true partner: under the pair's own geometry the row would be an inlier
    e, row = b("entry_N"), info["entry_N_row"]
    assert int(m0[e, row]) == N and e + 1 < k1.shape[0] and k1.is_contiguous()
    assert torch.equal(k1.reshape(-1, 2)[e * N + N], k1[e + 1, 0])
    x0 = ref.normalize_with_intrinsics(k0[e, row:row + 1], tr["K0"][e])
    x1 = ref.normalize_with_intrinsics(k1[e + 1, 0:1], tr["K1"][e])
    thr = ref.ransac_threshold(1.0, tr["K0"][e], tr["K1"][e])
    assert float(ref.sampson_error(x0, x1, ref.essential_from_Rt(tr["R"][e], tr["T"][e]))[0]) < 0.01 * thr * thr
    assert int(m0[e + 1, 0]) == -1
    # model counts of the hypothesis cases against the scorer's 256 lanes
    assert [(-(-h * 10 // 256), (h * 10) % 256) for h in mc.HYPOTHESIS_COUNTS] == [(1, 10), (1, 250), (2, 4), (5, 0)]


def test_restatement_of_relative_pose_on_small_scenes():
    k0, k1, m0, tr, out = geometry_ref.make_scene(1, 64, outliers=0.25, seed=600)
    seed = mc.seed_with_clean_samples([mc.clean_flags(m0[0], out[0])], 16)
    args = (k0[0], k1[0], m0[0], tr["K0"][0].float(), tr["K1"][0].float(), tr["R"][0], tr["T"][0])
    r = ref.relative_pose(*args, hypotheses=16, seed=seed)
    assert np.array_equal(r["inliers"], (~out[0]).numpy()) and r["num_inliers"] == r["ransac_inliers"] == int((~out[0]).sum())
    assert r["error"] < 0.05 and r["hypothesis"] >= 0 and abs(np.linalg.det(r["R"]) - 1) < 1e-12 and abs(np.linalg.norm(r["t"]) - 1) < 1e-12
    # the chosen candidate is the one in front of both cameras: the sign of t is resolved, not only its line
    assert float(tr["T"][0].numpy() @ r["t"]) > 0.99
    none = ref.relative_pose(k0[0], k1[0], torch.full((64,), -1), *args[3:])
    assert math.isinf(none["error"]) and none["hypothesis"] == -1 and not none["inliers"].any()
    cut = ref.relative_pose(*args, nk=4, hypotheses=4)
    assert math.isinf(cut["error"]) and cut["num_inliers"] == 0
    # the four candidates of kornia's decomposition: two rotations, both signs of t, all proper
    c = ref.decompose_essential(r["E"])
    assert len(c) == 4 and all(abs(np.linalg.det(R) - 1) < 1e-12 for R, _ in c)
    assert np.array_equal(c[0][0], c[1][0]) and np.array_equal(c[2][0], c[3][0]) and np.array_equal(c[0][1], -c[1][1])


# ------------------------------------------------------------------------------------------------ precision
@pytest.mark.parametrize("k", [3, 6, 10])
def test_precision_boundary_is_exact(k):
    k0, k1, m0, tr, d, at = mc.precision_boundary(k)
    assert k0.shape[1] == 257 and d == 2.0 ** (1 - 2 * k)
    dist, mask = ref.epipolar_distances(k0[0], k1[0], m0[0], tr["K0"][0], tr["K1"][0], tr["R"][0], tr["T"][0])
    assert int(mask.sum()) == 250 and int((dist == d).sum()) == at == 84 and int((dist == 0).sum()) == 250 - at
    up = float(np.nextafter(d, 1.0))
    assert ref.precision_counts(dist, 257, d)[0] == 250 - at and ref.precision_counts(dist, 257, up)[0] == 250


def test_precision_edges_by_hand():
    k0, k1, m0, tr, nk, expect = mc.precision_edges()
    M = k0.shape[1]
    for bq in range(k0.shape[0]):
        dist, mask = ref.epipolar_distances(k0[bq], k1[bq], m0[bq], tr["K0"][bq], tr["K1"][bq], tr["R"][bq], tr["T"][bq], int(nk[bq]))
        assert ref.precision_counts(dist, min(int(nk[bq]), M), 5e-4) == expect[bq], bq
    assert int(nk[0]) < M < int(nk[1]) and expect[3][1] != expect[3][2]
    assert int((m0[2] == k1.shape[1]).sum()) == 1 and not bool((m0[4] >= 0).any())


# ------------------------------------------------------------------------------------------------ the solver's text on the host
def test_solver_on_the_host_against_restatement(tmp_path):
    hipcc = next((c for c in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc") if c and os.path.exists(c)), None)
    if hipcc is None:
        pytest.fail("hipcc not found")
    exe = str(tmp_path / "five_point_host")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-std=c++17", "-O3", "-x", "hip", os.path.join(ROOT, "tests", "host", "five_point_host.cpp"),
                        "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    for family in mc.FAMILIES + mc.DEGENERATE:
        m, sols = solved(family)
        (tmp_path / "in.bin").write_bytes(np.int32(mc.P).tobytes() + m["x0"].tobytes() + m["x1"].tobytes())
        r = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, (family, r.returncode, r.stderr[-500:])
        raw = (tmp_path / "out.bin").read_bytes()
        ns = np.frombuffer(raw[:4 * mc.P], dtype=np.int32)
        E = np.frombuffer(raw[4 * mc.P:], dtype=np.float64).reshape(mc.P, 10, 3, 3)
        assert ns.min() >= 0 and ns.max() <= 10
        worst = 0.0
        for p in range(mc.P):
            got = list(E[p, :ns[p]])
            assert all(np.isfinite(g).all() for g in got) and valid(got, m["x0"][p], m["x1"][p]), (family, p)
            if family in mc.DEGENERATE:
                continue
            s, nd = sols[p]
            e_ref, e = mc.error_of_true(s, m["E"][p]), mc.error_of_true(got, m["E"][p])
            assert e <= max(10 * e_ref, 1e-9), (family, p, e, e_ref)
            assert nd or ns[p] == len(s), (family, p, ns[p], len(s))
            assert all(mc.error_of_true([got[i]], got[j]) > 1e-6 for i in range(len(got)) for j in range(i)), (family, p)
            worst = max(worst, e)
        print(f"{family}: host path, worst error of the true E {worst:.2e}, mean {ns.mean():.2f} solutions")
