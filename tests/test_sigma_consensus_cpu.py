"""CPU checks of sigma-consensus scoring (openglue_amd.geometry with scoring="sigma"): the float64 restatement
(tests/sigma_consensus_ref.py) against scipy, the check values and a quadrature of MAGSAC++'s rho, the q table the kernels interpolate
in, the robustness property on the restatement, the refusals, the three ABI entries and the scratch budget of csrc/sigma_consensus.hip
as the compiler reports it for gfx950.  No kernel is launched here."""
import inspect
import os
import re
import subprocess

import numpy as np
import pytest
import torch
from scipy import integrate, special

from openglue_amd import _lib, geometry
from openglue_amd import build as og_build
from tests import geometry_ref as gref
from tests import sigma_consensus_ref as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("og_fundamental_matrix_sc", "og_homography_sc", "og_sigma_consensus_eval")


# ------------------------------------------------------------------------------------------------ 1. the definition
def test_closed_forms_check_values_and_monotonicity():
    u = np.linspace(0.0, sc.U_MAX, 4001)
    assert np.abs(sc.closed_G15(u) - special.gammaincc(1.5, u) * special.gamma(1.5)).max() <= 1e-12
    assert np.abs(sc.closed_g25(u) - special.gammainc(2.5, u) * special.gamma(2.5)).max() <= 1e-12
    assert abs(sc.U_MAX - 6.6248) < 1e-12
    for t, q, w in ((0.25, 0.258884282595, 0.343210095719), (0.5, 0.051718422900, 0.081076330138)):
        assert abs(float(sc.quality(t)) - q) < 1e-11 and abs(float(sc.weight(t)) - w) < 1e-11, t
    t = np.linspace(0.0, 1.0, 100001)
    q, w = sc.quality(t), sc.weight(t)
    assert (np.diff(q) <= 0).all() and (np.diff(w) <= 0).all()
    assert q[0] == 1.0 and w[0] == 1.0 and abs(q[-1]) < 1e-15 and w[-1] == 0.0
    edge = np.array([-1.0, np.nextafter(1.0, 2.0), 2.0, np.inf, np.nan])
    assert not sc.quality(edge).any() and not sc.weight(edge).any()
    # sup t |q'(t)| = 0.4014: the factor the GPU tests turn a relative residual error into a quality error with
    tm = np.linspace(0.001, 0.999, 9981)
    slope = np.abs(tm * (sc.quality(tm + 1e-6) - sc.quality(tm - 1e-6)) / 2e-6).max()
    assert 0.4013 < slope < 0.4015, slope


def test_quality_is_magsac_rho_by_quadrature():
    """q(t) = 1 - rho(r) / rho(k sigma_max) with rho(r) = int_0^r x w(x) dx and w(x) = G(a, x^2 / (2 sigma_max^2)) - G(a, k^2 / 2), the
    loss of MAGSAC++ (Barath et al. 2020, eq. 5-7, constant factors dropped): integrated numerically, sigma_max = 1, r = k sqrt t."""
    wx = lambda x: special.gammaincc(sc.A, x * x / 2) - special.gammaincc(sc.A, sc.U_MAX)
    rho = lambda r: integrate.quad(lambda x: x * wx(x), 0.0, r, epsabs=1e-13, epsrel=1e-13)[0]
    total = rho(sc.K)
    for t in (0.0, 1e-4, 0.01, 0.1, 0.25, 0.5, 0.75, 0.9, 0.99, 1.0):
        assert abs((1.0 - rho(sc.K * np.sqrt(t)) / total) - float(sc.quality(t))) <= 1e-8, t
        assert abs(wx(sc.K * np.sqrt(t)) / wx(0.0) - float(sc.weight(t))) <= 1e-12, t


def test_fixed_point_rule_and_per_match_rule():
    e = np.array([0.0, 0.25, 0.5, 1.0, 1.0000001, np.inf, np.nan])
    assert sc.Q_of(e, 1.0) == 65536 + int(np.rint(65536 * 0.258884282595)) + int(np.rint(65536 * 0.051718422900))
    assert sc.Q_of(np.array([0.0, 0.0, 1e-30]), 0.0) == 2 * 65536      # threshold 0: t = 0 for e = 0, nothing else counts
    inl, w = sc.weights_of(e, 1.0)
    assert inl.tolist() == [True, True, True, True, False, False, False] and w[0] == 1.0 and not w[3:].any()


def test_q_table_header_holds_the_definition():
    """csrc/og_sigma_table.h (scripts/gen_sigma_table.py): 1025 entries, 65536 q(i / 1024) to one fp32 rounding, strictly decreasing
    from 65536 to 0; the chord between neighbours stays within 0.12 units of q, the interpolation error the kernels' bound counts."""
    text = open(os.path.join(og_build.CSRC, "og_sigma_table.h")).read()
    body = text[text.index("{", text.index("kSigmaQTable")) + 1:text.rindex("};")]
    tab = np.array([np.float32(v.strip().rstrip("f")) for v in body.split(",")], dtype=np.float32)
    assert tab.shape == (1025,) and tab[0] == 65536.0 and tab[-1] == 0.0 and (np.diff(tab) < 0).all()
    want = 65536 * sc.quality(np.arange(1025) / 1024)
    assert (np.abs(tab.astype(np.float64) - want) <= np.spacing(np.maximum(tab, np.float32(1e-3))).astype(np.float64)).all()
    mid = 65536 * sc.quality((np.arange(1024) + 0.5) / 1024)
    assert np.abs(0.5 * (tab[:-1].astype(np.float64) + tab[1:]) - mid).max() < 0.12


# ------------------------------------------------------------------------------------------------ 3. the property
def test_generous_threshold_costs_little_on_the_restatement():
    """make_scene(1, 300, outliers=0.3, noise=0.5, seed=100..107), 256 hypotheses, two refits; the error is the RMS Sampson distance of
    the noise-free true matches to the returned F, mean over the 8 scenes.  Measured with this restatement:
        threshold   plain count   sigma-consensus
        1 px        0.123         0.306
        2 px        0.096         0.127
        4 px        0.143         0.096
        8 px        0.994         0.097
        16 px       2.789         0.131
    Sigma-consensus is no worse than counting at 4, 8 and 16 px and under a quarter of it at 16 px; at 1 px (sigma_max = 0.27 px, below
    the 0.5 px noise) it is worse, the documented caveat."""
    mean = {}
    for thr in (1.0, 4.0, 8.0, 16.0):
        plain, sigma = [], []
        for seed in sc.PROPERTY_SEEDS:
            k0, k1, m0, p0, p1 = sc.property_scene(seed)
            a = gref.fundamental_matrix(k0, k1, m0, threshold=thr, hypotheses=sc.PROPERTY_H, refine=2)
            b = sc.fundamental_matrix_sigma(k0, k1, m0, threshold=thr, hypotheses=sc.PROPERTY_H, refine=2)
            plain.append(sc.rms_sampson(a["F"], p0, p1))
            sigma.append(sc.rms_sampson(b["F"], p0, p1))
        mean[thr] = (float(np.mean(plain)), float(np.mean(sigma)))
        print(f"threshold {thr:g} px: plain {mean[thr][0]:.3f}, sigma-consensus {mean[thr][1]:.3f}")
    for thr in (4.0, 8.0, 16.0):
        assert mean[thr][1] <= mean[thr][0], (thr, mean[thr])
    assert mean[16.0][1] < 0.25 * mean[16.0][0], mean[16.0]
    assert mean[1.0][1] > mean[1.0][0], mean[1.0]


def test_restatement_recovers_noise_free_scenes():
    k0, k1, m0, _, out = gref.make_scene(1, 120, outliers=0.3, seed=11, dtype=torch.float64)
    good = ~out[0].numpy()
    for refine in (0, 2):
        r = sc.fundamental_matrix_sigma(k0[0].numpy(), k1[0].numpy(), m0[0].numpy(), hypotheses=64, refine=refine)
        assert np.array_equal(r["inliers"], good) and r["num_inliers"] == int(good.sum())
        assert r["Q"] == 65536 * int(good.sum()) and r["quality"] == float(good.sum())
    from tests import homography_ref as href
    k0, k1, m0, _, out = href.make_scene(1, 120, outliers=0.3, seed=11, dtype=torch.float64)
    good = ~out[0].numpy()
    r = sc.homography_sigma(k0[0].numpy(), k1[0].numpy(), m0[0].numpy(), hypotheses=64)
    assert np.array_equal(r["inliers"], good) and abs(r["quality"] - good.sum()) < 1e-3
    few = sc.fundamental_matrix_sigma(k0[0].numpy()[:6], k1[0].numpy(), m0[0].numpy()[:6])
    assert few["best_model"] == -1 and few["Q"] == 0 and not few["F"].any()


# ------------------------------------------------------------------------------------------------ 4. refusals, ABI, scratch
def test_wrappers_refuse_bad_scoring_cpu_tensors_and_sizes():
    k, m = torch.zeros(2, 10, 2), torch.zeros(2, 10, dtype=torch.int64)
    for fn, args in ((geometry.fundamental_matrix, (k, k, m)), (geometry.homography, (k, k, m)), (geometry.find_fundamental, (k[0], k[0])),
                     (geometry.find_homography, (k[0], k[0]))):
        for bad in ("magsac", "Sigma", "", None, 1):
            with pytest.raises(ValueError, match="scoring must be"):
                fn(*args, scoring=bad)
        with pytest.raises(RuntimeError, match="GPU"):
            fn(*args, scoring="sigma")
    big, mb = torch.empty(1, 32769, 2, device="meta"), torch.empty(1, 32769, dtype=torch.int64, device="meta")
    ok, mo = torch.empty(1, 32768, 2, device="meta"), torch.empty(1, 32768, dtype=torch.int64, device="meta")
    for fn in (geometry.fundamental_matrix, geometry.homography):
        with pytest.raises(ValueError, match="at most 32768"):
            fn(big, big, mb, scoring="sigma")
        with pytest.raises(RuntimeError, match="GPU"):            # the largest M passes the size rule, and the plain path has none
            fn(ok, ok, mo, scoring="sigma")
        with pytest.raises(RuntimeError, match="GPU"):
            fn(big, big, mb)
        for kw in (dict(hypotheses=0), dict(hypotheses=-5), dict(refine=-1), dict(threshold=-1.0)):
            with pytest.raises(ValueError, match="hypotheses must be positive"):
                fn(k, k, m, scoring="sigma", **kw)
    with pytest.raises(RuntimeError, match="GPU"):
        geometry.sigma_consensus(torch.zeros(4))
    with pytest.raises(ValueError, match="between 1 and"):
        geometry.sigma_consensus(torch.zeros(0))


def test_entry_points_refuse_bad_sizes():
    """Before any launch: OG_E_INVALID (-1) as the plain entries and for a null quality, OG_E_SHAPE (-2) for m > 32768, OG_E_ALIGN (-3)."""
    lib = _lib.load()
    A = 0x10000                                       # never dereferenced: every call below is refused
    for name, too_many in (("og_fundamental_matrix_sc", 1024), ("og_homography_sc", 1025)):      # 3 B H, B H one step past 2^30
        def call(**kw):
            a = dict(batch=2, m=10, n=10, k0=A, k1=A, m0=A, nk=None, thr=1.0, hyp=8, refine=2, seed=0, off=0, M=A, inl=A, ninl=A, best=A,
                     quality=A, ws=A)
            a.update(kw)
            return getattr(lib, name)(a["batch"], a["m"], a["n"], a["k0"], a["k1"], a["m0"], a["nk"], a["thr"], a["hyp"], a["refine"],
                                      a["seed"], a["off"], a["M"], a["inl"], a["ninl"], a["best"], a["quality"], a["ws"], None)
        for bad in (dict(hyp=0), dict(hyp=-3), dict(batch=too_many, hyp=2 ** 20), dict(refine=-1), dict(batch=0), dict(M=None), dict(ws=None),
                    dict(k0=None), dict(m0=None), dict(best=None), dict(thr=-1.0), dict(quality=None)):
            assert call(**bad) == -1, (name, bad)
        assert call(m=32769) == -2 and call(m=2 ** 20) == -2, name
        assert call(ws=A + 8) == -3 and call(m=32768, ws=A + 8) == -3, name
    ev = lib.og_sigma_consensus_eval
    assert ev(0, A, A, A, None) == -1 and ev(-1, A, A, A, None) == -1 and ev(2 ** 30 + 1, A, A, A, None) == -1
    assert ev(4, None, A, A, None) == -1 and ev(4, A, None, A, None) == -1 and ev(4, A, A, None, None) == -1


def test_header_and_binding_hold_the_new_entries():
    header = open(os.path.join(ROOT, "include", "openglue_amd.h")).read()
    declared = set(re.findall(r"^\s*(?:int|size_t)\s+(og_\w+)\s*\(", header, flags=re.M))
    lib = _lib.load()
    for name in NAMES:
        assert name in declared and name in _lib.SYMBOLS and hasattr(lib, name), name
    assert re.search(r"#define OG_ABI_VERSION 14\b", header) and _lib.OG_ABI_VERSION == 14      # additive: no bump
    assert "sigma_consensus.hip" in og_build.SOURCES


def test_sigma_kernels_do_not_spill(tmp_path):
    """Every kernel of sigma_consensus.hip compiles for gfx950 with 0 bytes of scratch: sigma_eval_kernel is the only one.  The four
    sigma-consensus instances of the score and finish kernels are compiled in geometry.hip and homography.hip and checked, once each,
    by test_geometry_kernels_do_not_spill and test_homography_kernels_do_not_spill, as are the prep and solve kernels."""
    src = os.path.join(og_build.CSRC, "sigma_consensus.hip")
    r = subprocess.run([og_build._hipcc(), "--offload-arch=gfx950", "-std=c++17", "-O3", "-Rpass-analysis=kernel-resource-usage",
                        "--cuda-device-only", "-c", src, "-o", str(tmp_path / "s.o")], capture_output=True, text=True)
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
    for kernel in ("sigma_eval_kernel",):
        hits = [v for k, v in usage.items() if kernel in k]
        assert len(hits) == 1 and hits[0]["ScratchSize [bytes/lane]"] == 0, (kernel, usage)
    assert len(usage) == 1, usage                     # every RANSAC instance is in geometry.hip / homography.hip


# ------------------------------------------------------------------------------------------------ 5. the default
def test_default_scoring_is_inliers_and_adds_no_key(monkeypatch):
    """scoring defaults to "inliers" in all four signatures; with the device calls replaced by recorders, the default reaches the plain
    entry and returns today's four keys, "sigma" reaches the new entry and adds 'quality'."""
    for fn in (geometry.fundamental_matrix, geometry.homography):
        assert inspect.signature(fn).parameters["scoring"].default == "inliers"
    calls = []
    monkeypatch.setattr(_lib, "gpu_tensor", lambda t, name, dtype=torch.float32, convert=False: t)
    monkeypatch.setattr(_lib, "workspace", lambda nbytes, dev: (None, 0))
    monkeypatch.setattr(_lib, "call", lambda name, dev, *a: calls.append((name, len(a))))
    k, m = torch.zeros(2, 10, 2), torch.zeros(2, 10, dtype=torch.int64)
    for fn, plain, key in ((geometry.fundamental_matrix, "og_fundamental_matrix", "F"), (geometry.homography, "og_homography", "H")):
        for kw, entry, keys in (({}, plain, {key, "inliers", "num_inliers", "best_model"}),
                                (dict(scoring="inliers"), plain, {key, "inliers", "num_inliers", "best_model"}),
                                (dict(scoring="sigma"), plain + "_sc", {key, "inliers", "num_inliers", "best_model", "quality"})):
            calls.clear()
            r = fn(k, k, m, **kw)
            assert set(r) == keys and [c[0] for c in calls] == [entry], (kw, calls)
            assert calls[0][1] == (19 if "quality" in keys else 18)
    calls.clear()
    geometry.find_fundamental(k[0], k[0])
    geometry.find_homography(k[0], k[0], scoring="sigma")
    assert [c[0] for c in calls] == ["og_fundamental_matrix", "og_homography_sc"]
