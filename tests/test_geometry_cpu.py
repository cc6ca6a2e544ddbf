"""CPU checks of the geometric verification (openglue_amd.geometry): the float64 restatement (tests/geometry_ref.py) against ground
truth on noise-free scenes, its draws, the wrappers' refusals, the three ABI entries, and the scratch budget of csrc/geometry.hip
as the compiler reports it for gfx950.  No kernel is launched here."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from openglue_amd import _lib, geometry
from openglue_amd import build as og_build
from tests import geometry_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("og_fundamental_7pt", "og_fundamental_matrix_workspace_bytes", "og_fundamental_matrix")


def normalised_problem(k0, k1, F_px):
    """Seven pixel correspondences and the true pixel F -> Hartley-normalised points and the true F in that frame, unit norm."""
    (c0, s0), (c1, s1) = ref.hartley(k0), ref.hartley(k1)
    T0 = np.array([[s0, 0, -s0 * c0[0]], [0, s0, -s0 * c0[1]], [0, 0, 1.0]])
    T1 = np.array([[s1, 0, -s1 * c1[0]], [0, s1, -s1 * c1[1]], [0, 0, 1.0]])
    Ft = np.linalg.inv(T1).T @ F_px @ np.linalg.inv(T0)
    return (k0 - c0) * s0, (k1 - c1) * s1, Ft / np.linalg.norm(Ft)


def sign_free_error(F, Ft):
    return min(np.abs(F - Ft).max(), np.abs(F + Ft).max())


def test_restatement_solver_finds_the_true_F():
    """Noise-free float64 scenes: every solution of the restatement is a rank-2 matrix through the seven points to 1e-9 at unit
    norm, and one of them is the true F up to sign (1e-7: the conditioning of a minimal sample times the float64 rounding)."""
    P = 200
    k0, k1, _, tr, _ = ref.make_scene(P, 7, seed=3, dtype=torch.float64)
    counts = []
    for p in range(P):
        x0, x1, Ft = normalised_problem(k0[p].numpy(), k1[p].numpy(), tr["F"][p].numpy())
        sols, _ = ref.seven_point(x0, x1)
        counts.append(len(sols))
        assert 1 <= len(sols) <= 3, p
        A = ref.constraint_rows(x0, x1)
        for F in sols:
            assert abs(np.linalg.norm(F) - 1) < 1e-12
            assert abs(np.linalg.det(F)) <= 1e-9 and np.abs(A @ F.reshape(9)).max() <= 1e-9, p
        assert min(sign_free_error(F, Ft) for F in sols) < 1e-7, p
    assert set(counts) <= {1, 2, 3} and 3 in counts and 1 in counts


def test_restatement_ransac_recovers_noise_free_scene():
    k0, k1, m0, tr, out = ref.make_scene(1, 120, outliers=0.3, seed=11, dtype=torch.float64)
    for refine in (0, 2):
        r = ref.fundamental_matrix(k0[0].numpy(), k1[0].numpy(), m0[0].numpy(), hypotheses=64, refine=refine)
        assert np.array_equal(r["inliers"], ~out[0].numpy()) and r["num_inliers"] == int((~out[0]).sum())
        d = ref.sampson_sq(r["F"], k0[0].numpy()[~out[0].numpy()], k1[0].numpy()[~out[0].numpy()])
        assert d.max() < 1e-12
        assert abs(np.linalg.norm(r["F"]) - 1) < 1e-12 and r["F"].reshape(9)[np.abs(r["F"]).argmax()] > 0
    few = ref.fundamental_matrix(k0[0].numpy()[:6], k1[0].numpy(), m0[0].numpy()[:6])
    assert few["best_model"] == -1 and not few["inliers"].any() and not few["F"].any()


def test_restatement_draws_are_distinct_and_in_range():
    for n in (7, 8, 300):
        for h in range(50):
            pick = ref.draw_distinct(5, 2, h, n)
            assert len(set(pick)) == 7 and all(0 <= r < n for r in pick)
    assert ref.mix64(0) == 0xE220A8397B1DCDAF          # splitmix64's first output for state 0
    assert ref.draw_distinct(0, 0, 0, 300) != ref.draw_distinct(0, 1, 0, 300)


def test_wrappers_refuse_cpu_tensors_and_bad_shapes():
    k = torch.zeros(2, 10, 2)
    m = torch.zeros(2, 10, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="GPU"):
        geometry.fundamental_matrix(k, k, m)
    with pytest.raises(RuntimeError, match="GPU"):
        geometry.find_fundamental(k[0], k[0])
    with pytest.raises(RuntimeError, match="GPU"):
        geometry.fundamental_7pt(torch.zeros(3, 7, 2, dtype=torch.float64), torch.zeros(3, 7, 2, dtype=torch.float64))
    meta = lambda *s, **kw: torch.empty(*s, device="meta", **kw)      # not a GPU tensor either
    with pytest.raises(RuntimeError, match="GPU"):
        geometry.fundamental_matrix(meta(2, 10, 2), meta(2, 10, 2), meta(2, 10, dtype=torch.int64))
    with pytest.raises(RuntimeError, match="GPU"):
        geometry.fundamental_matrix(k.numpy(), k, m)
    with pytest.raises(RuntimeError, match="GPU"):
        geometry.fundamental_matrix(k, k, m, num_keypoints0=torch.zeros(2, dtype=torch.int32))


def bad_call(match, fn, *args, **kw):
    with pytest.raises(ValueError, match=match):
        fn(*args, **kw)


def test_wrappers_refuse_bad_shapes_and_arguments():
    """Every ValueError of geometry.py: shapes and scalar arguments are checked before the device, so these need none."""
    k, n8 = torch.zeros(2, 10, 2), torch.zeros(2, 8, 2)
    m = torch.zeros(2, 10, dtype=torch.int64)
    fm = geometry.fundamental_matrix
    for k0, k1 in ((torch.zeros(10, 2), torch.zeros(10, 2)), (torch.zeros(2, 10, 3), k), (k, torch.zeros(2, 8, 3)), (k, torch.zeros(2, 8)),
                   (k, torch.zeros(3, 8, 2)), (torch.zeros(0, 10, 2), torch.zeros(0, 8, 2)), (torch.zeros(2, 10, 2, 1), k)):
        bad_call(r"\[B, M, 2\]", fm, k0, k1, m)
    for m0 in (torch.zeros(2, 8, dtype=torch.int64), torch.zeros(2, 10, 1, dtype=torch.int64), torch.zeros(10, dtype=torch.int64),
               torch.zeros(3, 10, dtype=torch.int64)):
        bad_call(r"matches0 must be \[B, M\]", fm, k, n8, m0)
    for nk in (torch.zeros(3, dtype=torch.int32), torch.zeros(2, 1, dtype=torch.int32), torch.tensor(2, dtype=torch.int32)):
        bad_call(r"num_keypoints0 must be \[B\]", fm, k, n8, m, nk)
    for kw in (dict(hypotheses=0), dict(hypotheses=-5), dict(refine=-1), dict(threshold=-1.0), dict(threshold=float("nan"))):
        bad_call("hypotheses must be positive", fm, k, n8, m, **kw)
    bad_call(r"2\^30", fm, k, n8, m, hypotheses=2 ** 30 // 6 + 1)          # 3 * 2 * hypotheses one step past 2^30
    with pytest.raises(RuntimeError, match="GPU"):                          # the largest count passes the size rule
        fm(k, n8, m, hypotheses=2 ** 30 // 6)
    ff = geometry.find_fundamental
    for a, b in ((torch.zeros(9, 2), torch.zeros(8, 2)), (torch.zeros(9, 3), torch.zeros(9, 3)), (torch.zeros(1, 9, 2), torch.zeros(1, 9, 2)),
                 (torch.zeros(18), torch.zeros(18))):
        bad_call(r"\[K, 2\]", ff, a, b)
    f7 = geometry.fundamental_7pt
    z = lambda *s: torch.zeros(*s, dtype=torch.float64)
    for a, b in ((z(3, 8, 2), z(3, 8, 2)), (z(3, 7, 3), z(3, 7, 3)), (z(7, 2), z(7, 2)), (z(3, 7, 2), z(4, 7, 2)), (z(0, 7, 2), z(0, 7, 2)),
                 (torch.empty(2 ** 30 + 1, 7, 2, device="meta"), torch.empty(2 ** 30 + 1, 7, 2, device="meta"))):
        bad_call(r"\[count, 7, 2\]", f7, a, b)


def test_entry_points_refuse_bad_sizes():
    """The checks run before any launch: OG_E_INVALID (-1) for hypotheses <= 0, 3 * batch * hypotheses > 2^30, refine < 0, null
    pointers, more than 2^30 seven-point problems; OG_E_ALIGN (-3) for a workspace that is not 16-byte aligned; a workspace size of 0 for the same bad sizes."""
    lib = _lib.load()
    A = 0x10000                                       # never dereferenced: every call below is refused
    size = lib.og_fundamental_matrix_workspace_bytes
    assert size(4, 300, 512) > 0 and size(4, 300, 512) % 256 == 0
    assert size(1, 10, 0) == 0 and size(0, 10, 8) == 0 and size(1, -1, 8) == 0
    assert size(1, 10, 2 ** 30 // 3) > 0 and size(1, 10, 2 ** 30 // 3 + 1) == 0 and size(1024, 10, 2 ** 20) == 0

    def call(**kw):
        a = dict(batch=2, m=10, n=10, k0=A, k1=A, m0=A, nk=None, thr=1.0, hyp=8, refine=2, seed=0, off=0, F=A, inl=A, ninl=A, best=A, ws=A)
        a.update(kw)
        return lib.og_fundamental_matrix(a["batch"], a["m"], a["n"], a["k0"], a["k1"], a["m0"], a["nk"], a["thr"], a["hyp"], a["refine"],
                                         a["seed"], a["off"], a["F"], a["inl"], a["ninl"], a["best"], a["ws"], None)
    for bad in (dict(hyp=0), dict(hyp=-3), dict(batch=1024, hyp=2 ** 20), dict(refine=-1), dict(batch=0), dict(F=None), dict(ws=None),
                dict(k0=None), dict(m0=None), dict(best=None), dict(thr=-1.0)):
        assert call(**bad) == -1, bad
    assert call(ws=A + 8) == -3
    assert lib.og_fundamental_7pt(0, A, A, A, A, None) == -1 and lib.og_fundamental_7pt(4, None, A, A, A, None) == -1
    assert lib.og_fundamental_7pt(2 ** 30 + 1, A, A, A, A, None) == -1 and lib.og_fundamental_7pt(2 ** 31 - 1, A, A, A, A, None) == -1
    assert size(65536, 10, 1) > 0                     # the batch has no limit of its own


def test_header_and_binding_hold_the_new_entries():
    header = open(os.path.join(ROOT, "include", "openglue_amd.h")).read()
    declared = set(re.findall(r"^\s*(?:int|size_t)\s+(og_\w+)\s*\(", header, flags=re.M))
    lib = _lib.load()
    for name in NAMES:
        assert name in declared and name in _lib.SYMBOLS and hasattr(lib, name), name
    assert re.search(r"#define OG_ABI_VERSION 14\b", header) and _lib.OG_ABI_VERSION == 14      # additive: no bump
    assert "geometry.hip" in og_build.SOURCES


def test_geometry_kernels_do_not_spill(tmp_path):
    """Every kernel of geometry.hip compiles for gfx950 with 0 bytes of scratch: the solver's matrices and the refit's 45
    accumulators are indexed at compile time and stay in registers.  The six are the Fundamental instances of the RANSAC skeleton
    (og_ransac_hartley.h), each found exactly once; the two sigma-consensus instances (SC = 1), which test_sigma_consensus_cpu.py
    used to check in sigma_consensus.hip, are checked here."""
    src = os.path.join(og_build.CSRC, "geometry.hip")
    r = subprocess.run([og_build._hipcc(), "--offload-arch=gfx950", "-std=c++17", "-O3", "-Rpass-analysis=kernel-resource-usage",
                        "--cuda-device-only", "-c", src, "-o", str(tmp_path / "g.o")], capture_output=True, text=True)
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
    for kernel in ("ransac_prep_kernelINS_11FundamentalEE", "ransac_solve_kernelINS_11FundamentalEE",
                   "ransac_score_kernelINS_11FundamentalELi0E", "ransac_score_kernelINS_11FundamentalELi1E",
                   "ransac_finish_kernelINS_11FundamentalELi0E", "ransac_finish_kernelINS_11FundamentalELi1E"):
        hits = [v for k, v in usage.items() if kernel in k]
        assert len(hits) == 1 and hits[0]["ScratchSize [bytes/lane]"] == 0, (kernel, usage)
    assert len(usage) == 6, usage
