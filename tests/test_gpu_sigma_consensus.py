"""Sigma-consensus scoring on the MI355X (openglue_amd.geometry with scoring="sigma", csrc/sigma_consensus.hip) against the float64
restatement (tests/sigma_consensus_ref.py): the stage function on a dense grid, the RANSAC winner and the weighted refit on the noisy
scenes of tests/test_gpu_geometry.py / tests/test_gpu_homography.py, the robustness property, the edges, determinism and batching,
both for the fundamental matrix and the homography, and the plain path left where it was.

The band.  A quality computed in fp32 differs from the float64 one by at most DELTA per valid match: sup t |q'(t)| = 0.4014 times the
relative fp32 error of a residual, 4e-4 ("Precision"), plus 2^-16 for the fixed point (half a unit of rounding, 0.11
units of table interpolation, the FMA's rounding).  So over n matches two qualities may differ by n DELTA, and a winner may be any
model within that of the best."""
import functools

import numpy as np
import pytest
import torch

from openglue_amd import geometry
from tests import geometry_ref as gref
from tests import homography_ref as href
from tests import sigma_consensus_ref as sc
from tests.util import parity_note

pytestmark = pytest.mark.gpu

DELTA = 0.4015 * 4e-4 + 2.0 ** -16
NOISY_H = 256
KIND = {
    "F": dict(fn=geometry.fundamental_matrix, find=geometry.find_fundamental, ref=sc.fundamental_matrix_sigma, scene=gref.make_scene,
              scene_kw={}, Q=sc.Q_of_pixel_F, residual=lambda M, p0, p1: gref.sampson_sq(M, p0, p1), thresholds=(1.0, 8.0), min_n=7,
              refit_n=8, models=3, same=1e-6),
    "H": dict(fn=geometry.homography, find=geometry.find_homography, ref=sc.homography_sigma, scene=href.make_scene,
              scene_kw={"thr_px": 2.0}, Q=sc.Q_of_pixel_H, residual=lambda M, p0, p1: href.transfer_sq(M, p0, p1), thresholds=(2.0, 8.0),
              min_n=4, refit_n=5, models=1, same=1e-8),
}


def run(kind, k0, k1, m0, dev, nk=None, **kw):
    r = KIND[kind]["fn"](k0.to(dev), k1.to(dev), m0.to(dev), None if nk is None else nk.to(dev), scoring="sigma", **kw)
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in r.items()}


def check_outputs(kind, r, b, k0, k1, m0, thr, nk=None):
    """What every result must satisfy, pair b: the mask flags valid matches only, agrees with the float64 residual under the returned
    model outside 1 % of threshold^2 (at most 2 % of the matches inside), its sum is num_inliers, the model has unit norm with its
    largest entry positive (or is zero with best_model -1 and quality 0), and quality is the float64 Q / 65536 of the returned model
    within n DELTA.  Returns the number of valid matches."""
    M = r[kind][b].numpy()
    idx, p0, p1 = gref.valid_matches(k0.numpy(), k1.numpy(), m0.numpy(), nk)
    inl = r["inliers"][b].numpy()
    other = np.ones(len(inl), dtype=bool)
    other[idx] = False
    assert not inl[other].any() and int(r["num_inliers"][b]) == int(inl.sum())
    quality = float(r["quality"][b])
    if int(r["best_model"][b]) < 0:
        assert not M.any() and not inl.any() and quality == 0.0
        return len(idx)
    assert abs(np.linalg.norm(M) - 1) < 1e-12 and M.reshape(9)[np.abs(M).argmax()] > 0
    d2, t2 = KIND[kind]["residual"](M, p0, p1), thr * thr
    assert inl[idx][d2 < 0.99 * t2].all() and not inl[idx][d2 > 1.01 * t2].any()
    assert int(((d2 >= 0.99 * t2) & (d2 <= 1.01 * t2)).sum()) <= 0.02 * len(idx)
    want = sc.Q_float(d2, t2) / sc.UNIT
    assert abs(quality - want) <= len(idx) * DELTA + 1e-6 * want, (b, quality, want)      # 1e-6: quality is a float32
    assert 0.0 <= quality <= int(inl.sum())
    return len(idx)


# ------------------------------------------------------------------------------------------------ 1. the stage function
def test_stage_function_on_a_dense_grid(gpu_device):
    """2^20 + 1 evenly spaced t in [0, 1] and the edge values.  q is within one unit of rint(65536 q(t)) and does not increase along
    the grid.  w is within 1.5e-6 of the float64 weight: w = (sqrt(u) exp(-u) + (sqrt(pi) / 2) erfc(sqrt u) - G1) / 0.8826 in fp32 with
    u = t u_max <= 6.62, eps = 2^-24: the erfc term is at most 0.886 and OpenCL-conformant erfc is good to 16 ulp (0.886 x 32 eps =
    1.7e-6 before the division is the ceiling; the library's erfcf measures 1-2 ulp), the sqrt(u) exp(-u) term is at most 0.43 with
    (3 + 1 + 1 + 7) ulp from exp, sqrt, the product and u's own rounding through exp (u eps <= 7 eps), the subtraction and the division
    add 2 more on a quantity below 1: (0.886 x 16 + 0.43 x 12 + 2) x 2 eps / 0.8826 = 1.45e-6 < 1.5e-6.  A few 1e-7 is what is
    observed; the figure goes to the parity notes."""
    N = 1 << 20
    grid = (torch.arange(N + 1, dtype=torch.float64) / N).float()
    one = np.float32(1.0)
    edge = torch.tensor([0.0, float(np.float32(1e-45)), 1.0, float(np.nextafter(one, np.float32(0))), float(np.nextafter(one, np.float32(2))),
                         2.0, -1.0, float("inf"), float("nan")], dtype=torch.float32)
    t = torch.cat([grid, edge])
    q, w = geometry.sigma_consensus(t.to(gpu_device))
    torch.cuda.synchronize()
    q, w = q.cpu().numpy(), w.cpu().numpy()
    assert q.dtype == np.int64 and w.dtype == np.float32 and q.shape == w.shape == (N + 10,)
    t64 = t.numpy().astype(np.float64)
    q_ref, w_ref = np.rint(sc.UNIT * sc.quality(t64)), sc.weight(t64)
    dq, dw = np.abs(q - q_ref).max(), np.abs(w - w_ref).max()
    parity_note(f"sigma-consensus stage: {N + 1} grid points, max |q - rint(65536 q64)| {dq:.0f} units, "
                f"{int((q != q_ref).sum())} points off by one, max |w - w64| {dw:.2e}")
    assert dq <= 1, dq
    assert dw <= 1.5e-6, dw
    assert (np.diff(q[:N + 1]) <= 0).all(), int((np.diff(q[:N + 1]) > 0).sum())
    assert (np.diff(w[:N + 1]) <= 1e-6).all()
    eq, ew = q[N + 1:], w[N + 1:]
    assert eq[0] == 65536 and ew[0] == 1.0 and eq[1] == 65536 and abs(ew[1] - 1.0) <= 1.5e-6      # 0 and the smallest denormal
    assert eq[2] == 0 and 0.0 <= ew[2] <= 1.5e-6 and eq[3] == 0 and 0.0 <= ew[3] <= 1.5e-6          # 1 and the float below it
    assert not eq[4:].any() and not ew[4:].any()                                                   # above 1, 2, -1, inf, NaN
    # a shape of its own and a second, small launch
    q2, w2 = geometry.sigma_consensus(torch.tensor([[0.25, 0.5], [0.0, 1.5]], device=gpu_device))
    assert q2.shape == (2, 2) and q2[1].cpu().tolist() == [65536, 0]
    assert abs(int(q2[0, 0]) - int(q_ref[N // 4])) <= 1 and abs(int(q2[0, 1]) - int(q_ref[N // 2])) <= 1
    assert abs(float(w2[0, 0]) - 0.343210095719) < 1.5e-6 and abs(float(w2[0, 1]) - 0.081076330138) < 1.5e-6


# ------------------------------------------------------------------------------------------------ 2, 3. winner and weighted refit
@functools.lru_cache(maxsize=None)
def noisy(kind):
    """The noisy() scenes of the plain tests (four pairs of 300 matches and one of 1100, 0.5 px noise, 30 % outliers; the big pair spans
    two LDS chunks of the scorer) with the restatement's results per threshold at refine 0 and 2.  Computed once per model."""
    K = KIND[kind]
    small = K["scene"](4, 300, outliers=0.3, noise=0.5, seed=70, **K["scene_kw"])
    big = K["scene"](1, 1100, outliers=0.3, noise=0.5, seed=71, **K["scene_kw"])
    res = {}
    for thr in K["thresholds"]:
        for (k0, k1, m0, _, _), first in ((small, 0), (big, 4)):
            for b in range(k0.shape[0]):
                a = (k0[b].numpy(), k1[b].numpy(), m0[b].numpy())
                res[thr, first + b] = tuple(K["ref"](*a, threshold=thr, hypotheses=NOISY_H, refine=rf, pair=b) for rf in (0, 2))
    return small, big, res


@pytest.mark.parametrize("kind", ["F", "H"])
def test_winner_against_restatement(gpu_device, kind):
    K = KIND[kind]
    small, big, res = noisy(kind)
    for thr in K["thresholds"]:
        for (k0, k1, m0, _, _), first in ((small, 0), (big, 4)):
            r = run(kind, k0, k1, m0, gpu_device, threshold=thr, hypotheses=NOISY_H, refine=0)
            for b in range(k0.shape[0]):
                n = check_outputs(kind, r, b, k0[b], k1[b], m0[b], thr)
                want = res[thr, first + b][0]
                got_Q = K["Q"](r[kind][b].numpy(), k0[b].numpy(), k1[b].numpy(), m0[b].numpy(), thr, rounded=False) / sc.UNIT
                best, mine = int(r["best_model"][b]), want["best_model"]
                parity_note(f"sigma-consensus {kind}, winner, threshold {thr:g} px, pair {first + b}: float64 quality of the returned model "
                            f"{got_Q:.3f} (reported {float(r['quality'][b]):.3f}), restatement {want['ransac_Q'] / sc.UNIT:.3f}, band "
                            f"{n * DELTA:.3f}, models {best} / {mine}")
                assert got_Q >= want["ransac_Q"] / sc.UNIT - n * DELTA, (thr, first + b, got_Q, want["ransac_Q"] / sc.UNIT)
                if best // K["models"] == mine // K["models"]:
                    assert np.abs(r[kind][b].numpy() - want[kind]).max() <= K["same"], (thr, first + b)


@pytest.mark.parametrize("kind", ["F", "H"])
def test_weighted_refit(gpu_device, kind):
    K = KIND[kind]
    small, big, res = noisy(kind)
    for thr in K["thresholds"]:
        for (k0, k1, m0, _, _), first in ((small, 0), (big, 4)):
            r0 = run(kind, k0, k1, m0, gpu_device, threshold=thr, hypotheses=NOISY_H, refine=0)
            r2 = run(kind, k0, k1, m0, gpu_device, threshold=thr, hypotheses=NOISY_H, refine=2)
            assert torch.equal(r0["best_model"], r2["best_model"])
            for b in range(k0.shape[0]):
                n = check_outputs(kind, r2, b, k0[b], k1[b], m0[b], thr)
                q0, q2, want = float(r0["quality"][b]), float(r2["quality"][b]), res[thr, first + b][1]["quality"]
                parity_note(f"sigma-consensus {kind}, weighted refit, threshold {thr:g} px, pair {first + b}: quality {q0:.3f} -> {q2:.3f} "
                            f"(restatement {res[thr, first + b][0]['quality']:.3f} -> {want:.3f}), inliers {int(r0['num_inliers'][b])} -> "
                            f"{int(r2['num_inliers'][b])}")
                assert q2 >= q0, (thr, first + b, q2, q0)
                assert q2 >= want - n * DELTA, (thr, first + b, q2, want)


# ------------------------------------------------------------------------------------------------ 4. the property
def test_generous_threshold_costs_little(gpu_device):
    """The 8 scenes of tests/test_sigma_consensus_cpu.py at 4, 8 and 16 px, 256 hypotheses, two refits: the mean RMS Sampson distance of
    the noise-free true matches to the GPU's F is within 10 % of the restatement's mean at each threshold."""
    for thr in (4.0, 8.0, 16.0):
        got, want = [], []
        for seed in sc.PROPERTY_SEEDS:
            k0, k1, m0, p0, p1 = sc.property_scene(seed)
            r = run("F", *(torch.from_numpy(a)[None] for a in (k0, k1, m0)), gpu_device, threshold=thr, hypotheses=sc.PROPERTY_H, refine=2)
            got.append(sc.rms_sampson(r["F"][0].numpy(), p0, p1))
            want.append(sc.rms_sampson(sc.fundamental_matrix_sigma(k0, k1, m0, threshold=thr, hypotheses=sc.PROPERTY_H, refine=2)["F"], p0, p1))
        g, w = float(np.mean(got)), float(np.mean(want))
        parity_note(f"sigma-consensus F, 0.5 px noise, 30 % outliers, threshold {thr:g} px: mean RMS Sampson distance of the true matches "
                    f"{g:.4f} px (restatement {w:.4f})")
        assert abs(g - w) <= 0.1 * w, (thr, g, w)


# ------------------------------------------------------------------------------------------------ 5. edges
def edge_batch(kind):
    """M = 70 rows, N = 64, seven pairs: no match; one fewer than a minimal sample; exactly a minimal sample; one more than that
    (enough for a refit); 12 chance matches; ragged with holes and entries >= N; every point on one spot."""
    K = KIND[kind]
    M, N, k = 70, 64, K["min_n"]
    k0, k1, _, _, _ = K["scene"](7, M, seed=60)
    k1 = k1[:, :N]
    g = torch.Generator().manual_seed(61)
    m0 = torch.arange(M).repeat(7, 1)
    m0[m0 >= N] = 1000                                        # entries >= N are no matches
    m0[0] = -1
    m0[1, k - 1:] = -1
    m0[2, :20] = -1
    m0[2, 20 + k:] = -1
    m0[3, :30] = -1
    m0[3, 30 + k + 1:] = -1
    k0[4] = torch.rand(M, 2, generator=g) * torch.tensor([639.0, 479.0])
    m0[4, 12:] = -1
    m0[5][torch.rand(M, generator=g) < 0.3] = -1
    k0[6], k1[6] = torch.tensor([100.0, 120.0]), torch.tensor([50.0, 60.0])
    nk = torch.tensor([M, M, M, M, M, 68, M], dtype=torch.int32)      # pair 5: rows 64..67 hold entries >= N, 68 and 69 are cut
    return k0, k1, m0, nk


@pytest.mark.parametrize("kind", ["F", "H"])
def test_edges_small(gpu_device, kind):
    K = KIND[kind]
    k, thr = K["min_n"], K["thresholds"][0]
    k0, k1, m0, nk = edge_batch(kind)
    a = run(kind, k0, k1, m0, gpu_device, nk=nk, threshold=thr, hypotheses=86, refine=2)
    a0 = run(kind, k0, k1, m0, gpu_device, nk=nk, threshold=thr, hypotheses=86, refine=0)
    for r in (a, a0):
        for key, v in r.items():
            assert bool(torch.isfinite(v.double()).all()), key
        for b in range(7):
            check_outputs(kind, r, b, k0[b], k1[b], m0[b], thr, int(nk[b]))
    for b in (0, 1, 6):                                       # no model: zero, -1, quality 0 (check_outputs) in both runs
        assert int(a["best_model"][b]) == -1 and int(a0["best_model"][b]) == -1
    # a minimal sample: its matches fit exactly, q = 1 each, and there is nothing to refit
    assert int(a["num_inliers"][2]) == k and bool(a["inliers"][2, 20:20 + k].all()) and float(a["quality"][2]) == float(k)
    assert all(torch.equal(a[key][2], a0[key][2]) for key in a)
    # one more (noise-free): all of them inliers at q = 1, before and after the refit
    for r in (a, a0):
        assert int(r["num_inliers"][3]) == k + 1 and abs(float(r["quality"][3]) - (k + 1)) < 1e-3
    for b in range(7):
        assert float(a["quality"][b]) >= float(a0["quality"][b])
    idx5, _, _ = gref.valid_matches(k0[5].numpy(), k1[5].numpy(), m0[5].numpy(), 68)
    assert k < len(idx5) < 64 and int(a["num_inliers"][5]) == len(idx5) and abs(float(a["quality"][5]) - len(idx5)) < 1e-3
    # threshold 0 on the noise-free ragged pair: only a residual of exactly 0 counts, each at q = 1; finite, consistent outputs
    z = run(kind, k0[5:6], k1[5:6], m0[5:6], gpu_device, nk=nk[5:6], threshold=0.0, hypotheses=86)
    assert all(bool(torch.isfinite(v.double()).all()) for v in z.values())
    assert int(z["num_inliers"][0]) == int(z["inliers"][0].sum()) and float(z["quality"][0]) == float(z["num_inliers"][0])
    assert (int(z["best_model"][0]) >= 0) == bool(z[kind][0].any())


@pytest.mark.parametrize("kind", ["F", "H"])
def test_edges_more_pairs_than_a_grid_is_high(gpu_device, kind):
    """65540 pairs of min_n + 1 noise-free matches, one hypothesis: the pair index runs along the grid's x extent.  Every sample is
    clean, so every pair keeps all its matches at q = 1, and the last pair equals a call of its own."""
    K = KIND[kind]
    n, thr = K["min_n"] + 1, K["thresholds"][0] if kind == "F" else 3.0
    k0, k1, m0, _, _ = K["scene"](4, n, seed=63)
    B = 65540
    K0, K1, M0 = k0.repeat(B // 4, 1, 1), k1.repeat(B // 4, 1, 1), m0.repeat(B // 4, 1)
    r = run(kind, K0, K1, M0, gpu_device, threshold=thr, hypotheses=1)
    assert bool((r["num_inliers"] == n).all()) and bool(r["inliers"].all()) and bool((r["best_model"] >= 0).all())
    assert bool(torch.isfinite(r[kind]).all()) and bool(((r["quality"] - n).abs() < 1e-3).all())
    one = run(kind, K0[-1:], K1[-1:], M0[-1:], gpu_device, threshold=thr, hypotheses=1, pair_offset=B - 1)
    for key in r:
        assert torch.equal(one[key][0], r[key][B - 1]), key
    check_outputs(kind, r, B - 1, K0[-1], K1[-1], M0[-1], thr)


# ------------------------------------------------------------------------------------------------ 6. determinism and batching
@pytest.mark.parametrize("kind", ["F", "H"])
def test_deterministic_and_batched_equals_per_pair(gpu_device, kind):
    K = KIND[kind]
    B, M = 4, 300
    k0, k1, m0, _, _ = K["scene"](B, M, outliers=0.3, noise=0.5, seed=80, **K["scene_kw"])
    g = torch.Generator().manual_seed(81)
    m0[torch.rand(B, M, generator=g) < 0.3] = -1
    m0[2, 3:] = -1                                     # too few matches for a model
    nk = torch.randint(M // 2, M + 1, (B,), generator=g, dtype=torch.int32)
    kw = dict(hypotheses=200, seed=9, threshold=4.0)
    a = run(kind, k0, k1, m0, gpu_device, nk=nk, **kw)
    b2 = run(kind, k0, k1, m0, gpu_device, nk=nk, **kw)
    assert set(a) == {kind, "inliers", "num_inliers", "best_model", "quality"}
    for key in a:
        assert torch.equal(a[key], b2[key]), key
    assert int(a["best_model"][2]) == -1 and float(a["quality"][2]) == 0.0 and int(a["best_model"][0]) >= 0
    for b in range(B):
        one = run(kind, k0[b:b + 1], k1[b:b + 1], m0[b:b + 1], gpu_device, nk=nk[b:b + 1], pair_offset=b, **kw)
        for key in a:
            assert torch.equal(one[key][0], a[key][b]), (b, key)
        keep = (m0[b] >= 0) & (torch.arange(M) < int(nk[b]))
        Mc, inl = K["find"](k0[b][keep].to(gpu_device), k1[b][m0[b][keep]].to(gpu_device), pair_offset=b, scoring="sigma", **kw)
        want = a[kind][b]
        if kind == "H":
            want = want / want[2, 2] if int(a["best_model"][b]) >= 0 else torch.zeros(3, 3, dtype=torch.float64)
        assert torch.equal(Mc.cpu(), want) and torch.equal(inl.cpu(), a["inliers"][b][keep]), b
        check_outputs(kind, a, b, k0[b], k1[b], m0[b], 4.0, int(nk[b]))


# ------------------------------------------------------------------------------------------------ 8. nothing existing moved
@pytest.mark.parametrize("kind", ["F", "H"])
def test_plain_scoring_is_the_default_path(gpu_device, kind):
    K = KIND[kind]
    small, big, _ = noisy(kind)
    for k0, k1, m0, _, _ in (small, big):
        args = (k0.to(gpu_device), k1.to(gpu_device), m0.to(gpu_device))
        for refine in (0, 2):
            a = K["fn"](*args, threshold=K["thresholds"][0], hypotheses=NOISY_H, refine=refine)
            b = K["fn"](*args, threshold=K["thresholds"][0], hypotheses=NOISY_H, refine=refine, scoring="inliers")
            assert set(a) == set(b) == {kind, "inliers", "num_inliers", "best_model"}
            for key in a:
                assert torch.equal(a[key], b[key]), key
