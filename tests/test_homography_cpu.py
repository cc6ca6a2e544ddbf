"""CPU checks of the homography path (openglue_amd.geometry.homography, openglue_amd.metrics.Homography*): the float64 restatement
(tests/homography_ref.py) against ground truth on noise-free scenes, its draws and its validity rule, the wrappers' refusals, the
five ABI entries, and the scratch budget of csrc/homography.hip as the compiler reports it for gfx950.  No kernel is launched here."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from openglue_amd import _lib, geometry, metrics
from openglue_amd import build as og_build
from tests import homography_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("og_homography_4pt", "og_homography_workspace_bytes", "og_homography", "og_homography_precision", "og_homography_corner_error")


def normalised_problem(k0, k1, H_px):
    """Pixel correspondences and the true pixel H -> Hartley-normalised points and the true H in that frame, unit norm, signed."""
    (c0, s0), (c1, s1) = ref.hartley(k0), ref.hartley(k1)
    T0 = np.array([[s0, 0, -s0 * c0[0]], [0, s0, -s0 * c0[1]], [0, 0, 1.0]])
    T1 = np.array([[s1, 0, -s1 * c1[0]], [0, s1, -s1 * c1[1]], [0, 0, 1.0]])
    return (k0 - c0) * s0, (k1 - c1) * s1, ref.unit_signed(T1 @ H_px @ np.linalg.inv(T0))


def test_restatement_solver_holds_the_constraints():
    """Noise-free float64 minimal samples: the restatement's H is a unit-norm matrix with its largest entry positive that holds the
    eight DLT constraints to 1e-9 and maps the four points onto their partners."""
    P = 200
    k0, k1, _, Ht, _ = ref.make_scene(P, 4, seed=3, dtype=torch.float64)
    kept = 0
    for p in range(P):
        x0, x1, _ = normalised_problem(k0[p].numpy(), k1[p].numpy(), Ht[p].numpy())
        Hm = ref.four_point(x0, x1)
        if Hm is None:                                   # only the orientation rule may refuse an exact sample
            assert not ref.sample_is_oriented(x0, x1), p
            continue
        kept += 1
        assert abs(np.linalg.norm(Hm) - 1) < 1e-12 and Hm.reshape(9)[np.abs(Hm).argmax()] > 0
        assert np.abs(ref.dlt_rows(x0, x1) @ Hm.reshape(9)).max() <= 1e-9, p
        assert np.sqrt(ref.transfer_sq(Hm, x0, x1)).max() < 1e-7, p
    assert kept >= 0.9 * P


def test_restatement_ransac_recovers_noise_free_scene():
    k0, k1, m0, Ht, out = ref.make_scene(1, 120, outliers=0.3, seed=11, dtype=torch.float64)
    good = ~out[0].numpy()
    for refine in (0, 2):
        r = ref.homography(k0[0].numpy(), k1[0].numpy(), m0[0].numpy(), hypotheses=64, refine=refine)
        assert np.array_equal(r["inliers"], good) and r["num_inliers"] == int(good.sum())
        assert np.sqrt(ref.transfer_sq(r["H"], k0[0].numpy()[good], k1[0].numpy()[good])).max() < 1e-9
        assert abs(np.linalg.norm(r["H"]) - 1) < 1e-12 and r["H"].reshape(9)[np.abs(r["H"]).argmax()] > 0
        assert ref.corner_error(r["H"], Ht[0].numpy(), ref.W, ref.H) < 1e-9
    few = ref.homography(k0[0].numpy()[:3], k1[0].numpy(), m0[0].numpy()[:3])
    assert few["best_model"] == -1 and not few["inliers"].any() and not few["H"].any()
    assert ref.corner_error(few["H"], Ht[0].numpy(), ref.W, ref.H) == np.inf


def test_restatement_draws_are_distinct_and_in_range():
    for n in (4, 5, 300):
        for h in range(50):
            pick = ref.draw_distinct(5, 2, h, n, k=4)
            assert len(set(pick)) == 4 and all(0 <= r < n for r in pick)
    assert ref.mix64(0) == 0xE220A8397B1DCDAF          # splitmix64's first output for state 0
    assert ref.draw_distinct(0, 0, 0, 300, k=4) != ref.draw_distinct(0, 1, 0, 300, k=4)


def test_restatement_refuses_collinear_and_flipped_samples():
    x0 = np.array([[-1.0, -0.8], [1.0, -0.9], [0.9, 1.1], [-1.1, 1.0]])
    Ht = np.array([[1.0, 0.1, 0.05], [-0.05, 0.9, 0.1], [0.02, -0.03, 1.0]])
    x1 = ref.project(Ht, x0)
    assert ref.four_point(x0, x1) is not None
    col0 = x0.copy()
    col0[2] = 0.5 * (x0[0] + x0[1])                      # three collinear points in image 0
    assert ref.four_point(col0, ref.project(Ht, col0)) is None
    flip = x1.copy()
    flip[[0, 1]] = flip[[1, 0]]                          # two partners exchanged: the quadrilateral folds over, a triple changes sign
    assert ref.four_point(x0, flip) is None
    same = x0.copy()
    same[1] = same[0]                                    # two identical points
    assert ref.four_point(same, ref.project(Ht, same)) is None


def test_wrappers_refuse_cpu_tensors():
    k = torch.zeros(2, 10, 2)
    m = torch.zeros(2, 10, dtype=torch.int64)
    tr = {"H": torch.eye(3).repeat(2, 1, 1)}
    z = lambda *s: torch.zeros(*s, dtype=torch.float64)
    meta = lambda *s, **kw: torch.empty(*s, device="meta", **kw)      # not a GPU tensor either
    calls = [
        lambda: geometry.homography(k, k, m),
        lambda: geometry.find_homography(k[0], k[0]),
        lambda: geometry.homography_4pt(z(3, 4, 2), z(3, 4, 2)),
        lambda: geometry.homography(meta(2, 10, 2), meta(2, 10, 2), meta(2, 10, dtype=torch.int64)),
        lambda: geometry.homography(k.numpy(), k, m),
        lambda: geometry.homography(k, k, m, num_keypoints0=torch.zeros(2, dtype=torch.int32)),
        lambda: metrics.homography_precision(k, k, m, tr),
        lambda: metrics.homography_precision(meta(2, 10, 2), meta(2, 10, 2), meta(2, 10, dtype=torch.int64), {"H": meta(2, 3, 3)}),
        lambda: metrics.homography_error(z(2, 3, 3), torch.zeros(2, 3, 3), (640, 480)),
        lambda: metrics.HomographyAccuracy().update(k[0], k[0], {"H": torch.eye(3)}, 12),
        lambda: metrics.HomographyAccuracy().update_batch(k, k, m, tr),
        lambda: metrics.HomographyAUC([3, 5, 10], 3.0, (640, 480)).update(k[0], k[0], {"H": torch.eye(3)}),
        lambda: metrics.HomographyAUC([3, 5, 10], 3.0, (640, 480)).update_batch(k, k, m, tr),
    ]
    for i, fn in enumerate(calls):
        with pytest.raises(RuntimeError, match="GPU"):
            fn()
            pytest.fail(f"call {i} did not raise")


def bad_call(match, fn, *args, **kw):
    with pytest.raises(ValueError, match=match):
        fn(*args, **kw)


def test_wrappers_refuse_bad_shapes_and_arguments():
    """Every ValueError of the homography wrappers: shapes and scalar arguments are checked before the device, so these need none."""
    k, n8 = torch.zeros(2, 10, 2), torch.zeros(2, 8, 2)
    m = torch.zeros(2, 10, dtype=torch.int64)
    tr = {"H": torch.eye(3).repeat(2, 1, 1)}
    hm = geometry.homography
    hp = lambda k0, k1, m0, *a, **kw: metrics.homography_precision(k0, k1, m0, tr, *a, **kw)
    for fn in (hm, hp):
        for k0, k1 in ((torch.zeros(10, 2), torch.zeros(10, 2)), (torch.zeros(2, 10, 3), k), (k, torch.zeros(2, 8, 3)), (k, torch.zeros(2, 8)),
                       (k, torch.zeros(3, 8, 2)), (torch.zeros(0, 10, 2), torch.zeros(0, 8, 2)), (torch.zeros(2, 10, 2, 1), k)):
            bad_call(r"\[B, M, 2\]", fn, k0, k1, m)
        for m0 in (torch.zeros(2, 8, dtype=torch.int64), torch.zeros(2, 10, 1, dtype=torch.int64), torch.zeros(10, dtype=torch.int64),
                   torch.zeros(3, 10, dtype=torch.int64)):
            bad_call(r"matches0 must be \[B, M\]", fn, k, n8, m0)
        for nk in (torch.zeros(3, dtype=torch.int32), torch.zeros(2, 1, dtype=torch.int32), torch.tensor(2, dtype=torch.int32)):
            bad_call(r"num_keypoints0 must be \[B\]", fn, k, n8, m, nk)
    for kw in (dict(hypotheses=0), dict(hypotheses=-5), dict(refine=-1), dict(threshold=-1.0), dict(threshold=float("nan"))):
        bad_call("hypotheses must be positive", hm, k, n8, m, **kw)
    bad_call(r"2\^30", hm, k, n8, m, hypotheses=2 ** 29 + 1)                # 2 * hypotheses one step past 2^30
    with pytest.raises(RuntimeError, match="GPU"):                          # the largest count passes the size rule
        hm(k, n8, m, hypotheses=2 ** 29)
    for thr in (-1.0, float("nan")):
        bad_call("threshold must be non-negative", hp, k, n8, m, threshold=thr)
    for Hbad in (torch.eye(3), torch.zeros(3, 3, 3), torch.zeros(2, 9)):
        bad_call(r"transformation\['H'\] must be \[2, 3, 3\]", metrics.homography_precision, k, n8, m, {"H": Hbad})
        bad_call(r"transformation\['H'\] must be \[2, 3, 3\]", metrics.HomographyAUC([5], 3.0, (640, 480)).update_batch, k, n8, m, {"H": Hbad})
    fh = geometry.find_homography
    for a, b in ((torch.zeros(9, 2), torch.zeros(8, 2)), (torch.zeros(9, 3), torch.zeros(9, 3)), (torch.zeros(1, 9, 2), torch.zeros(1, 9, 2)),
                 (torch.zeros(18), torch.zeros(18))):
        bad_call(r"\[K, 2\]", fh, a, b)
    h4 = geometry.homography_4pt
    z = lambda *s: torch.zeros(*s, dtype=torch.float64)
    for a, b in ((z(3, 5, 2), z(3, 5, 2)), (z(3, 4, 3), z(3, 4, 3)), (z(4, 2), z(4, 2)), (z(3, 4, 2), z(4, 4, 2)), (z(0, 4, 2), z(0, 4, 2)),
                 (torch.empty(2 ** 30 + 1, 4, 2, device="meta"), torch.empty(2 ** 30 + 1, 4, 2, device="meta"))):
        bad_call(r"\[count, 4, 2\]", h4, a, b)
    he = metrics.homography_error
    for a, b in ((z(3, 3), torch.zeros(3, 3)), (z(2, 3, 3), torch.zeros(3, 3, 3)), (z(2, 9), torch.zeros(2, 9)), (z(0, 3, 3), torch.zeros(0, 3, 3))):
        bad_call(r"\[B, 3, 3\]", he, a, b, (640, 480))
    for size in ((0, 480), (640, -1)):
        bad_call("image_size", he, z(2, 3, 3), torch.zeros(2, 3, 3), size)


def test_entry_points_refuse_bad_sizes():
    """The checks run before any launch: OG_E_INVALID (-1) for hypotheses <= 0, batch * hypotheses > 2^30, refine < 0, a negative or
    NaN threshold, null pointers, a count outside [1, 2^30]; OG_E_ALIGN (-3) for a workspace that is not 16-byte aligned; a workspace
    size of 0 for the same bad sizes."""
    lib = _lib.load()
    A = 0x10000                                       # never dereferenced: every call below is refused
    size = lib.og_homography_workspace_bytes
    assert size(4, 300, 512) > 0 and size(4, 300, 512) % 256 == 0
    assert size(1, 10, 0) == 0 and size(0, 10, 8) == 0 and size(1, -1, 8) == 0 and size(-2, 10, 8) == 0
    assert size(1, 10, 2 ** 30) > 0 and size(1, 10, 2 ** 30 + 1) == 0 and size(1024, 10, 2 ** 20 + 1) == 0 and size(1024, 10, 2 ** 20) > 0
    assert size(65536, 10, 1) > 0                     # the batch has no limit of its own

    def call(**kw):
        a = dict(batch=2, m=10, n=10, k0=A, k1=A, m0=A, nk=None, thr=3.0, hyp=8, refine=2, seed=0, off=0, H=A, inl=A, ninl=A, best=A, ws=A)
        a.update(kw)
        return lib.og_homography(a["batch"], a["m"], a["n"], a["k0"], a["k1"], a["m0"], a["nk"], a["thr"], a["hyp"], a["refine"],
                                 a["seed"], a["off"], a["H"], a["inl"], a["ninl"], a["best"], a["ws"], None)
    for bad in (dict(hyp=0), dict(hyp=-3), dict(batch=1024, hyp=2 ** 20 + 1), dict(refine=-1), dict(batch=0), dict(batch=-1), dict(H=None),
                dict(ws=None), dict(k0=None), dict(k1=None), dict(m0=None), dict(inl=None), dict(ninl=None), dict(best=None), dict(thr=-1.0),
                dict(thr=float("nan")), dict(n=-1), dict(m=-1)):
        assert call(**bad) == -1, bad
    assert call(ws=A + 8) == -3
    f4 = lib.og_homography_4pt
    assert f4(0, A, A, A, A, None) == -1 and f4(-1, A, A, A, A, None) == -1 and f4(2 ** 30 + 1, A, A, A, A, None) == -1
    assert f4(2 ** 31 - 1, A, A, A, A, None) == -1
    for i in range(4):
        args = [A, A, A, A]
        args[i] = None
        assert f4(4, *args, None) == -1, i

    def prec(**kw):
        a = dict(batch=2, m=10, n=10, k0=A, k1=A, m0=A, nk=None, H=A, thr=3.0, p=A, s=A, c=A)
        a.update(kw)
        return lib.og_homography_precision(a["batch"], a["m"], a["n"], a["k0"], a["k1"], a["m0"], a["nk"], a["H"], a["thr"], a["p"], a["s"],
                                           a["c"], None)
    for bad in (dict(batch=0), dict(m=-1), dict(n=-1), dict(k0=None), dict(k1=None), dict(m0=None), dict(H=None), dict(p=None), dict(s=None),
                dict(c=None), dict(thr=-1.0), dict(thr=float("nan"))):
        assert prec(**bad) == -1, bad
    ce = lib.og_homography_corner_error
    assert ce(0, A, A, 640, 480, A, None) == -1 and ce(2, None, A, 640, 480, A, None) == -1 and ce(2, A, None, 640, 480, A, None) == -1
    assert ce(2, A, A, 640, 480, None, None) == -1 and ce(2, A, A, 0, 480, A, None) == -1 and ce(2, A, A, 640, 0, A, None) == -1


def test_header_and_binding_hold_the_new_entries():
    header = open(os.path.join(ROOT, "include", "openglue_amd.h")).read()
    declared = set(re.findall(r"^\s*(?:int|size_t)\s+(og_\w+)\s*\(", header, flags=re.M))
    lib = _lib.load()
    for name in NAMES:
        assert name in declared and name in _lib.SYMBOLS and hasattr(lib, name), name
    assert re.search(r"#define OG_ABI_VERSION 14\b", header) and _lib.OG_ABI_VERSION == 14      # additive: no bump
    assert "homography.hip" in og_build.SOURCES
    for name in ("homography", "find_homography", "homography_4pt"):
        assert callable(getattr(geometry, name))
    for name in ("homography_precision", "homography_error", "HomographyAccuracy", "HomographyAUC"):
        assert callable(getattr(metrics, name))


def test_homography_kernels_do_not_spill(tmp_path):
    """Every kernel of homography.hip compiles for gfx950 with 0 bytes of scratch: the solver's 8 x 9 system and the refit's 45
    accumulators are indexed at compile time and stay in registers.  Six are the Homography instances of the RANSAC skeleton
    (og_ransac_hartley.h), two the metrics, each found exactly once; the two sigma-consensus instances (SC = 1), which
    test_sigma_consensus_cpu.py used to check in sigma_consensus.hip, are checked here."""
    src = os.path.join(og_build.CSRC, "homography.hip")
    r = subprocess.run([og_build._hipcc(), "--offload-arch=gfx950", "-std=c++17", "-O3", "-Rpass-analysis=kernel-resource-usage",
                        "--cuda-device-only", "-c", src, "-o", str(tmp_path / "h.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    usage, name = {}, None
    for line in r.stderr.splitlines():
        mm = re.search(r"Function Name: (\S+)", line)
        if mm:
            name = mm.group(1)
        mm = re.search(r"(VGPRs|AGPRs|ScratchSize \[bytes/lane\]): (\d+)", line)
        if mm and name:
            usage.setdefault(name, {})[mm.group(1)] = int(mm.group(2))
    print(usage)
    for kernel in ("ransac_prep_kernelINS_10HomographyEE", "ransac_solve_kernelINS_10HomographyEE",
                   "ransac_score_kernelINS_10HomographyELi0E", "ransac_score_kernelINS_10HomographyELi1E",
                   "ransac_finish_kernelINS_10HomographyELi0E", "ransac_finish_kernelINS_10HomographyELi1E",
                   "hm_precision_kernel", "hm_corner_error_kernel"):
        hits = [v for k, v in usage.items() if kernel in k]
        assert len(hits) == 1 and hits[0]["ScratchSize [bytes/lane]"] == 0, (kernel, usage)
    assert len(usage) == 8, usage
