"""The homography path on the MI355X (openglue_amd.geometry.homography / find_homography / homography_4pt, openglue_amd.metrics
HomographyAccuracy / HomographyAUC, csrc/homography.hip) against the float64 restatement (tests/homography_ref.py): the four-point
solver on exact minimal problems, RANSAC on noise-free and noisy scenes, the consistency of the mask with the returned H, the edges,
the refit, determinism and batching, the metrics, and the path from homography_pairs through SIFT and the labels."""
import functools

import numpy as np
import pytest
import torch

from openglue_amd import geometry, metrics
from tests import homography_ref as ref
from tests.util import parity_note

pytestmark = pytest.mark.gpu

THR = 3.0          # pixels: cv2.findHomography's customary threshold, the noise-free scenes
NOISY_THR = 2.0    # the noisy scenes: at 0.5 px noise 0.07 % of the true matches lie within 1 % of 2^2 px^2 (1.1 % at 1 px)


def run(k0, k1, m0, dev, nk=None, **kw):
    r = geometry.homography(k0.to(dev), k1.to(dev), m0.to(dev), None if nk is None else nk.to(dev), **kw)
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in r.items()}


def scenes(specs, **kw):
    """One pair per (outliers, seed) -> a batch."""
    parts = [ref.make_scene(1, outliers=o, seed=s, **kw) for o, s in specs]
    return tuple(torch.cat([p[i] for p in parts]) for i in range(5))


def seed_with_clean_samples(clean, hypotheses, pair_offset=0):
    """The first RANSAC seed under which every pair draws at least one all-inlier sample.  clean: per pair, the truth (True =
    inlier) over the pair's valid matches in index order.  Decided from the restatement's draws alone, before any kernel runs."""
    for seed in range(200):
        if all(any(all(c[r] for r in ref.draw_distinct(seed, pair_offset + b, h, len(c), k=4)) for h in range(hypotheses))
               for b, c in enumerate(clean)):
            return seed
    raise AssertionError("no seed below 200 draws a clean sample for every pair")


def band_check(Hm, k0, k1, m0, inliers, nk=None, thr=THR, label=None):
    """With the returned H in float64, a valid match with d^2 < 0.99 thr^2 is flagged, one with d^2 > 1.01 thr^2 is not, and nothing
    else is flagged; at most 2 % of the valid matches lie in between.  Returns (matches in between, valid matches, d^2 of the valid
    matches, their index); with `label` the number in between goes to the parity notes."""
    idx, p0, p1 = ref.valid_matches(k0.numpy(), k1.numpy(), m0.numpy(), nk)
    inl = inliers.numpy()
    other = np.ones(len(inl), dtype=bool)
    other[idx] = False
    assert not inl[other].any(), "a keypoint without a valid match is flagged"
    d2 = ref.transfer_sq(Hm.numpy(), p0, p1) if Hm.numpy().any() else np.full(len(idx), np.inf)
    t2 = thr * thr
    assert inl[idx][d2 < 0.99 * t2].all(), int((~inl[idx][d2 < 0.99 * t2]).sum())
    assert not inl[idx][d2 > 1.01 * t2].any(), int(inl[idx][d2 > 1.01 * t2].sum())
    between = int(((d2 >= 0.99 * t2) & (d2 <= 1.01 * t2)).sum())
    if label:
        parity_note(f"{label}: {between} of {len(idx)} matches within 1 % of the threshold^2")
    assert between <= 0.02 * max(len(idx), 1), (between, len(idx))
    return between, len(idx), d2, idx


def unit_and_signed(Hm):
    Hm = Hm.numpy()
    return abs(np.linalg.norm(Hm) - 1) < 1e-12 and Hm.reshape(9)[np.abs(Hm).argmax()] > 0


def normalised(k0, k1, H_px):
    (c0, s0), (c1, s1) = ref.hartley(k0), ref.hartley(k1)
    T0 = np.array([[s0, 0, -s0 * c0[0]], [0, s0, -s0 * c0[1]], [0, 0, 1.0]])
    T1 = np.array([[s1, 0, -s1 * c1[0]], [0, s1, -s1 * c1[1]], [0, 0, 1.0]])
    return (k0 - c0) * s0, (k1 - c1) * s1, ref.unit_signed(T1 @ H_px @ np.linalg.inv(T0))


# ------------------------------------------------------------------------------------------------ 1. minimal solver
def test_four_point_solver(gpu_device):
    P = 2049
    k0, k1, _, Ht, _ = ref.make_scene(P, 4, seed=3, dtype=torch.float64)
    x0, x1, Hn = np.zeros((P, 4, 2)), np.zeros((P, 4, 2)), np.zeros((P, 3, 3))
    for p in range(P):
        x0[p], x1[p], Hn[p] = normalised(k0[p].numpy(), k1[p].numpy(), Ht[p].numpy())
    Hg, ns = geometry.homography_4pt(torch.from_numpy(x0).to(gpu_device), torch.from_numpy(x1).to(gpu_device))
    torch.cuda.synchronize()
    Hg, ns = Hg.cpu().numpy(), ns.cpu().numpy()
    assert np.isfinite(Hg).all() and ns.min() >= 0 and ns.max() <= 1
    worst, solved = 0.0, 0
    for p in range(P):
        want = ref.four_point(x0[p], x1[p])
        assert (want is not None) == bool(ns[p]), (p, ns[p])
        if not ns[p]:
            assert not Hg[p].any(), p                         # the unused slot is zero
            continue
        solved += 1
        assert abs(np.linalg.norm(Hg[p]) - 1) < 1e-9 and Hg[p].reshape(9)[np.abs(Hg[p]).argmax()] > 0
        assert np.abs(ref.dlt_rows(x0[p], x1[p]) @ Hg[p].reshape(9)).max() <= 1e-9, p
        e_ref, e_gpu = np.abs(want - Hn[p]).max(), np.abs(Hg[p] - Hn[p]).max()
        worst = max(worst, e_gpu)
        assert e_gpu <= max(10 * e_ref, 1e-9), (p, e_gpu, e_ref)
    parity_note(f"four-point solver: {P} problems, {solved} solved, worst error of the true normalised H {worst:.2e}")
    assert solved >= 0.9 * P
    # degenerate samples: a finite answer, 0 solutions, the slot zero
    d0, d1 = np.repeat(x0[:1], 3, 0), np.repeat(x1[:1], 3, 0)
    d0[0, 1], d1[0, 1] = d0[0, 0], d1[0, 0]                   # two identical points
    d0[1, 2] = 0.5 * (d0[1, 0] + d0[1, 1])                    # three collinear in image 0
    d1[1] = ref.project(Hn[0], d0[1])
    d1[2, [0, 1]] = d1[2, [1, 0]]                             # a flipped triple
    Hd, nd = geometry.homography_4pt(torch.from_numpy(d0).to(gpu_device), torch.from_numpy(d1).to(gpu_device))
    assert bool(torch.isfinite(Hd).all()) and not bool(Hd.any()) and not bool(nd.any())


# ------------------------------------------------------------------------------------------------ 2, 3. noise-free RANSAC, band check
def test_ransac_noise_free(gpu_device):
    k0, k1, m0, Ht, out = scenes([(0.0, 10), (0.3, 11), (0.6, 12), (0.3, 13)], n=300)
    B, Hy = 4, 300                                            # two workgroups per pair, the second with 44 live lanes
    seed = seed_with_clean_samples([(~out[b]).tolist() for b in range(B)], Hy)
    r = run(k0, k1, m0, gpu_device, hypotheses=Hy, seed=seed)
    for b in range(B):
        assert torch.equal(r["inliers"][b], ~out[b]), (b, int((r["inliers"][b] != ~out[b]).sum()))
        assert int(r["num_inliers"][b]) == int((~out[b]).sum())
        assert unit_and_signed(r["H"][b])
        band_check(r["H"][b], k0[b], k1[b], m0[b], r["inliers"][b], label=f"homography, noise-free RANSAC pair {b}")
        want = ref.homography(k0[b].numpy(), k1[b].numpy(), m0[b].numpy(), hypotheses=Hy, seed=seed, pair=b)
        assert want["best_model"] == int(r["best_model"][b]), (b, want["best_model"], int(r["best_model"][b]))
        good = (~out[b]).numpy()
        p0, p1 = k0[b].double().numpy()[good], k1[b].double().numpy()[good]
        d_gpu = np.sqrt(ref.transfer_sq(r["H"][b].numpy(), p0, p1).max())
        d_ref = np.sqrt(ref.transfer_sq(want["H"], p0, p1).max())
        parity_note(f"homography, noise-free RANSAC pair {b}: largest transfer distance of the true matches {d_gpu:.2e} px "
                    f"(restatement {d_ref:.2e})")
        assert d_gpu <= 4 * d_ref, (b, d_gpu, d_ref)


# ------------------------------------------------------------------------------------------------ 4. edges
def test_edges_small(gpu_device):
    """M = 70 rows (fewer than a workgroup has threads), N = 64: no match, 3 matches, exactly 4, pure chance, ragged with holes and
    entries >= N, every point on one spot.  86 hypotheses (not a multiple of 256), refine 2 and 0, then a single hypothesis."""
    M, N = 70, 64
    k0, k1, _, Ht, _ = ref.make_scene(6, M, seed=60)
    k1 = k1[:, :N]
    g = torch.Generator().manual_seed(61)
    m0 = torch.arange(M).repeat(6, 1)
    m0[m0 >= N] = 1000                                        # entries >= N are no matches
    m0[0] = -1
    m0[1, 3:] = -1
    m0[2, :20] = -1
    m0[2, 24:] = -1                                           # exactly 4
    k0[3] = torch.rand(M, 2, generator=g) * torch.tensor([639.0, 479.0])     # 12 chance matches
    m0[3, 12:] = -1
    m0[4][torch.rand(M, generator=g) < 0.3] = -1
    k0[5], k1[5] = torch.tensor([100.0, 120.0]), torch.tensor([50.0, 60.0])
    nk = torch.tensor([M, M, M, M, 68, M], dtype=torch.int32)     # pair 4: rows 64..67 hold entries >= N, 68 and 69 are cut
    a = run(k0, k1, m0, gpu_device, nk=nk, hypotheses=86, refine=2)
    a0 = run(k0, k1, m0, gpu_device, nk=nk, hypotheses=86, refine=0)
    for k, v in a.items():
        assert bool(torch.isfinite(v.double()).all()), k
    for b in (0, 1, 5):
        assert int(a["best_model"][b]) == -1 and int(a["num_inliers"][b]) == 0 and not bool(a["inliers"][b].any())
        assert not bool(a["H"][b].any())
    assert int(a["num_inliers"][2]) == 4 and bool(a["inliers"][2, 20:24].all()) and int(a["inliers"][2].sum()) == 4
    assert all(torch.equal(a[k][2], a0[k][2]) for k in a)     # exactly 4 matches: below 5 inliers nothing is refitted
    assert 0 <= int(a["best_model"][2]) < 86 and unit_and_signed(a["H"][2])
    for b in range(6):
        assert int(a["num_inliers"][b]) == int(a["inliers"][b].sum()) and int(a0["num_inliers"][b]) == int(a0["inliers"][b].sum())
        assert int(a["num_inliers"][b]) >= int(a0["num_inliers"][b])
        has = int(a["best_model"][b]) >= 0
        assert has == bool(a["H"][b].any()) and (has or int(a["num_inliers"][b]) == 0)
        band_check(a["H"][b], k0[b], k1[b], m0[b], a["inliers"][b], int(nk[b]))
    # pair 4: noise-free matches among the holes; its valid ones are all inliers once a sample is clean
    idx4, _, _ = ref.valid_matches(k0[4].numpy(), k1[4].numpy(), m0[4].numpy(), 68)
    assert 4 < len(idx4) < 64 and int(a["num_inliers"][4]) == len(idx4)
    # one hypothesis: on a noise-free pair without outliers the one sample is clean
    want = ref.homography(k0[4].numpy(), k1[4].numpy(), m0[4].numpy(), 68, hypotheses=1, pair=0)
    assert want["best_model"] == 0 and want["num_inliers"] == len(idx4)
    one = run(k0[4:5], k1[4:5], m0[4:5], gpu_device, nk=nk[4:5], hypotheses=1)
    assert int(one["best_model"][0]) == 0 and int(one["num_inliers"][0]) == len(idx4)
    assert torch.equal(torch.nonzero(one["inliers"][0])[:, 0], torch.from_numpy(idx4))


# ------------------------------------------------------------------------------------------------ 5. two LDS chunks
def test_edges_more_matches_than_one_chunk(gpu_device):
    """M = 1100 with more than 1024 valid matches: the scorer stages its points in two chunks."""
    k0, k1, m0, Ht, out = ref.make_scene(1, 1100, outliers=0.3, seed=62)
    m0[0, 5] = -1
    clean = [[bool(v) for i, v in enumerate((~out[0]).tolist()) if i != 5]]
    seed = seed_with_clean_samples(clean, 86)
    r = run(k0, k1, m0, gpu_device, hypotheses=86, seed=seed)
    want = ~out[0]
    want[5] = False
    assert torch.equal(r["inliers"][0], want), int((r["inliers"][0] != want).sum())
    assert int(r["num_inliers"][0]) == int(want.sum())
    band_check(r["H"][0], k0[0], k1[0], m0[0], r["inliers"][0])


# ------------------------------------------------------------------------------------------------ 6. grid extent
def test_edges_more_pairs_than_a_grid_is_high(gpu_device):
    """65540 pairs of 5 noise-free matches, one hypothesis: the pair index runs along the grid's x extent, which has room for it
    (y ends at 65535).  Whichever four of its five matches a pair draws, the restatement keeps all five (checked here for the four
    distinct pairs the batch repeats), so every pair keeps 5, and the last pair equals a call of its own."""
    k0, k1, m0, _, _ = ref.make_scene(4, 5, seed=63)
    for b in range(4):
        idx, p0, p1 = ref.valid_matches(k0[b].numpy(), k1[b].numpy(), m0[b].numpy())
        (c0, s0), (c1, s1) = ref.hartley(p0), ref.hartley(p1)
        x0, x1 = (p0 - c0) * s0, (p1 - c1) * s1
        for leave in range(5):
            pick = [i for i in range(5) if i != leave]
            Hm = ref.four_point(x0[pick], x1[pick])
            assert Hm is not None and ref.transfer_sq(Hm, x0, x1).max() < 0.01 * (THR * s1) ** 2, (b, leave)
    B = 65540
    K0, K1, M0 = k0.repeat(B // 4, 1, 1), k1.repeat(B // 4, 1, 1), m0.repeat(B // 4, 1)
    r = run(K0, K1, M0, gpu_device, hypotheses=1)
    assert bool((r["num_inliers"] == 5).all()) and bool(r["inliers"].all()) and bool((r["best_model"] == 0).all())
    assert bool(torch.isfinite(r["H"]).all())
    one = run(K0[-1:], K1[-1:], M0[-1:], gpu_device, hypotheses=1, pair_offset=B - 1)
    for k in r:
        assert torch.equal(one[k][0], r[k][B - 1]), k
    band_check(r["H"][B - 1], K0[-1], K1[-1], M0[-1], r["inliers"][B - 1])


# ------------------------------------------------------------------------------------------------ 7. noisy scenes
NOISY_H = 256


@functools.lru_cache(maxsize=None)
def noisy():
    """Four pairs of 300 matches and one of 1100, 0.5 px noise, 30 % outliers, with the restatement's results at refine 0 and 2
    and the inlier count of the true H.  Computed once, read by both tests."""
    small = ref.make_scene(4, 300, outliers=0.3, noise=0.5, seed=70, thr_px=NOISY_THR)
    big = ref.make_scene(1, 1100, outliers=0.3, noise=0.5, seed=71, thr_px=NOISY_THR)
    res = []
    for k0, k1, m0, Ht, _ in (small, big):
        for b in range(k0.shape[0]):
            a = (k0[b].numpy(), k1[b].numpy(), m0[b].numpy())
            r0 = ref.homography(*a, threshold=NOISY_THR, hypotheses=NOISY_H, refine=0, pair=b)
            r2 = ref.homography(*a, threshold=NOISY_THR, hypotheses=NOISY_H, refine=2, pair=b)
            true = int((ref.transfer_sq(Ht[b].numpy(), k0[b].double().numpy(), k1[b].double().numpy()) <= NOISY_THR ** 2).sum())
            res.append((r0, r2, true))
    return small, big, res


def test_winner_against_restatement(gpu_device):
    t2 = NOISY_THR ** 2
    band = lambda d: (d >= 0.99 * t2) & (d <= 1.01 * t2)
    small, big, res = noisy()
    for (k0, k1, m0, Ht, _), first in ((small, 0), (big, 4)):
        r = run(k0, k1, m0, gpu_device, threshold=NOISY_THR, hypotheses=NOISY_H, refine=0)
        for b in range(k0.shape[0]):
            between, n, d2, _ = band_check(r["H"][b], k0[b], k1[b], m0[b], r["inliers"][b], thr=NOISY_THR)
            c = int((d2 <= t2).sum())
            d2_ref = ref.transfer_sq(res[first + b][0]["H"], k0[b].double().numpy(), k1[b].double().numpy())
            k = int((band(d2) | band(d2_ref)).sum())
            c_ref = res[first + b][0]["ransac_inliers"]
            parity_note(f"homography, RANSAC winner pair {first + b}: fp64 inliers of the returned H {c}, restatement {c_ref}, {k} matches "
                        f"in the 1 % band ({between} under the returned H), hypotheses {int(r['best_model'][b])} / {res[first + b][0]['best_model']}")
            assert c >= c_ref - k, (first + b, c, c_ref, k)
            assert int(r["num_inliers"][b]) == int(r["inliers"][b].sum())


def test_refit(gpu_device):
    small, big, res = noisy()
    corners = np.array([[0, 0], [0, ref.H - 1], [ref.W - 1, 0], [ref.W - 1, ref.H - 1]], dtype=np.float64)
    worst_gpu, worst_ref, worst_min = 0.0, 0.0, 0.0
    for (k0, k1, m0, Ht, _), first in ((small, 0), (big, 4)):
        r0 = run(k0, k1, m0, gpu_device, threshold=NOISY_THR, hypotheses=NOISY_H, refine=0)
        r2 = run(k0, k1, m0, gpu_device, threshold=NOISY_THR, hypotheses=NOISY_H, refine=2)
        assert torch.equal(r0["best_model"], r2["best_model"])
        for b in range(k0.shape[0]):
            n0, n2 = int(r0["num_inliers"][b]), int(r2["num_inliers"][b])
            assert n2 >= n0, (first + b, n2, n0)
            band_check(r2["H"][b], k0[b], k1[b], m0[b], r2["inliers"][b], thr=NOISY_THR, label=f"homography, refit pair {first + b}")
            assert unit_and_signed(r2["H"][b]) and n2 == int(r2["inliers"][b].sum())
            _, ref2, true = res[first + b]
            ratio, ratio_ref = n2 / true, ref2["num_inliers"] / true
            assert ratio >= ratio_ref - 0.02, (first + b, ratio, ratio_ref)
            e_min = ref.corner_error(r0["H"][b].numpy(), Ht[b].numpy(), ref.W, ref.H)
            e_gpu = ref.corner_error(r2["H"][b].numpy(), Ht[b].numpy(), ref.W, ref.H)
            e_ref = ref.corner_error(ref2["H"], Ht[b].numpy(), ref.W, ref.H)
            same = bool(np.array_equal(r2["inliers"][b].numpy(), ref2["inliers"]))
            apart = np.sqrt(((ref.project(r2["H"][b].numpy(), corners) - ref.project(ref2["H"], corners)) ** 2).sum(1)).max()
            parity_note(f"homography, refit pair {first + b}: inliers / true-H inliers {n0 / true:.3f} -> {ratio:.3f} (restatement "
                        f"{ratio_ref:.3f}); mean corner error {e_min:.3f} -> {e_gpu:.3f} px (restatement {e_ref:.3f}); mask "
                        f"{'equal' if same else 'differs'}, corners {apart:.2e} px apart")
            if same:                                          # fp64 least squares over the same rows: only the summation order differs
                assert apart <= 1e-6, (first + b, apart)
            else:
                assert e_gpu <= 2 * e_ref, (first + b, e_gpu, e_ref)
            worst_gpu, worst_ref, worst_min = max(worst_gpu, e_gpu), max(worst_ref, e_ref), max(worst_min, e_min)
    parity_note(f"homography, refit, 0.5 px noise, 30 % outliers, {NOISY_H} hypotheses, threshold {NOISY_THR} px: worst mean corner error "
                f"{worst_min:.3f} px (minimal model) -> {worst_gpu:.3f} px (two refits), restatement {worst_ref:.3f} px")


# ------------------------------------------------------------------------------------------------ 8. determinism and batching
def test_deterministic_and_batched_equals_per_pair(gpu_device):
    B, M = 4, 300
    k0, k1, m0, Ht, _ = ref.make_scene(B, M, outliers=0.3, noise=0.5, seed=80, thr_px=NOISY_THR)
    g = torch.Generator().manual_seed(81)
    m0[torch.rand(B, M, generator=g) < 0.3] = -1
    m0[2, 3:] = -1                                     # too few matches for a model
    nk = torch.randint(M // 2, M + 1, (B,), generator=g, dtype=torch.int32)
    kw = dict(hypotheses=200, seed=9, threshold=NOISY_THR)
    a = run(k0, k1, m0, gpu_device, nk=nk, **kw)
    b2 = run(k0, k1, m0, gpu_device, nk=nk, **kw)
    for k in a:
        assert torch.equal(a[k], b2[k]), k
    assert int(a["best_model"][2]) == -1 and int(a["best_model"][0]) >= 0
    for b in range(B):
        one = run(k0[b:b + 1], k1[b:b + 1], m0[b:b + 1], gpu_device, nk=nk[b:b + 1], pair_offset=b, **kw)
        for k in a:
            assert torch.equal(one[k][0], a[k][b]), (b, k)
        # the same matches without the padding rows and holes around them
        keep = (m0[b] >= 0) & (torch.arange(M) < int(nk[b]))
        Hc, inl = geometry.find_homography(k0[b][keep].to(gpu_device), k1[b][m0[b][keep]].to(gpu_device), pair_offset=b, **kw)
        want = a["H"][b] / a["H"][b][2, 2] if int(a["best_model"][b]) >= 0 else torch.zeros(3, 3, dtype=torch.float64)
        assert torch.equal(Hc.cpu(), want), b
        assert torch.equal(inl.cpu(), a["inliers"][b][keep]), b
        band_check(a["H"][b], k0[b], k1[b], m0[b], a["inliers"][b], int(nk[b]), thr=NOISY_THR, label=f"homography, batched pair {b}")


# ------------------------------------------------------------------------------------------------ 9. metrics
def test_metrics(gpu_device):
    dev = gpu_device
    B, M = 4, 200
    k0, k1, m0, Ht, out = ref.make_scene(B, M, outliers=0.3, noise=1.0, seed=90)
    g = torch.Generator().manual_seed(91)
    m0[torch.rand(B, M, generator=g) < 0.3] = -1
    m0[1] = -1                                         # an empty pair
    m0[2, 3:] = -1                                     # too few matches for a model
    nk = torch.tensor([M, M, M, 150], dtype=torch.int32)
    H32 = Ht.float()
    want = [ref.precision(k0[b].numpy(), k1[b].numpy(), m0[b].numpy(), H32[b].numpy(), int(nk[b]), THR) for b in range(B)]
    for w in want:                                     # no match so close to the threshold that float64 rounding could decide it
        assert not (np.abs(w[3] - THR) < 1e-6).any()
    assert 0 < want[0][2] < len(want[0][3]) and want[1][2] == 0 and len(want[1][3]) == 0
    tr = {"type": ["perspective"] * B, "H": H32.to(dev)}
    r = metrics.homography_precision(k0.to(dev), k1.to(dev), m0.to(dev), tr, nk.to(dev), THR)
    for b in range(B):
        assert int(r["num_correct"][b]) == want[b][2], b
        assert float(r["precision"][b]) == float(want[b][0]) and float(r["matching_score"][b]) == float(want[b][1]), b
    one = metrics.homography_precision(k0[3:].to(dev), k1[3:].to(dev), m0[3:].to(dev), {"H": H32[3:].to(dev)}, nk[3:].to(dev), THR)
    assert all(torch.equal(one[k][0], r[k][3]) for k in r)
    # HomographyAccuracy: per-pair updates (compacted matches, the detected count) equal one update_batch
    acc_b, acc_p = metrics.HomographyAccuracy(THR), metrics.HomographyAccuracy(THR)
    acc_b.update_batch(k0.to(dev), k1.to(dev), m0.to(dev), tr, nk.to(dev))
    auc_b, auc_p = (metrics.HomographyAUC([3, 5, 10], THR, (ref.W, ref.H), hypotheses=128, seed=4) for _ in range(2))
    auc_b.update_batch(k0.to(dev), k1.to(dev), m0.to(dev), tr, nk.to(dev))
    for b in range(B):
        keep = (m0[b] >= 0) & (torch.arange(M) < int(nk[b]))
        a0, a1 = k0[b][keep].to(dev), k1[b][m0[b][keep]].to(dev)
        acc_p.update(a0, a1, {"H": H32[b].to(dev)}, int(nk[b]))
        auc_p(a0, a1, {"H": H32[b].to(dev)})
    cb, cp = acc_b.compute(), acc_p.compute()
    assert set(cb) == {"Precision", "Matching Score"}
    assert torch.equal(torch.cat(acc_b.precision), torch.cat(acc_p.precision))
    assert torch.equal(torch.cat(acc_b.matching_score), torch.cat(acc_p.matching_score))
    assert float(cb["Precision"]) == float(cp["Precision"]) and float(cb["Matching Score"]) == float(cp["Matching Score"])
    assert abs(float(cb["Precision"]) - np.mean([float(w[0]) for w in want])) < 1e-6
    # HomographyAUC: batched equals per pair; no model counts as inf; the curve is pose_auc's
    eb, ep = torch.cat(auc_b.corner_errors).cpu(), torch.cat(auc_p.corner_errors).cpu()
    assert torch.equal(eb, ep) and auc_b._pairs == auc_p._pairs == B
    assert bool(torch.isinf(eb[1])) and bool(torch.isinf(eb[2])) and bool(torch.isfinite(eb[[0, 3]]).all())
    est = run(k0, k1, m0, dev, nk=nk, threshold=THR, hypotheses=128, seed=4)
    e_ref = torch.tensor([ref.corner_error(est["H"][b].numpy(), H32[b].double().numpy(), ref.W, ref.H) for b in range(B)])
    assert torch.equal(torch.isinf(e_ref), torch.isinf(eb))
    fin = torch.isfinite(eb)
    assert bool((eb[fin].double() - e_ref[fin]).abs().max() <= 1e-6 * e_ref[fin].max())       # float32 output of a float64 mean
    got = auc_b.compute()
    assert set(got) == {"AUC@3px", "AUC@5px", "AUC@10px"}
    want_auc = metrics.pose_auc(e_ref.float().to(dev), [3, 5, 10])
    for t in (3, 5, 10):
        assert abs(float(got[f"AUC@{t}px"]) - float(want_auc[f"AUC@{t}deg"])) <= 1e-6, t
        assert float(got[f"AUC@{t}px"]) == float(auc_p.compute()[f"AUC@{t}px"])
    assert 0 < float(got["AUC@10px"]) <= 0.5                   # two of the four pairs have no model
    parity_note(f"homography metrics: corner errors {[round(float(v), 4) for v in eb]} px, AUC@3/5/10px "
                f"{[round(float(got[f'AUC@{t}px']), 4) for t in (3, 5, 10)]}")
    err = metrics.homography_error(est["H"].to(dev), H32.to(dev), (ref.W, ref.H)).cpu()
    assert torch.equal(err, eb)
    # find_homography: cv2's return order and scale
    keep = m0[0] >= 0
    Hc, mask = geometry.find_homography(k0[0][keep].to(dev), k1[0][m0[0][keep]].to(dev), threshold=THR, hypotheses=128, seed=4)
    assert float(Hc[2, 2]) == 1.0 and Hc.dtype == torch.float64
    assert torch.equal(mask.cpu(), est["inliers"][0][keep])
    none, mask0 = geometry.find_homography(k0[0][:3].to(dev), k1[0][:3].to(dev))
    assert not bool(none.any()) and not bool(mask0.any())


# ------------------------------------------------------------------------------------------------ 10. end to end
def test_end_to_end_from_pairs_sift_and_labels(gpu_device):
    """pairs.homography_pairs on two 240 x 320 frames -> SIFT -> the labels of supervision.generate_gt_matches as matches0.  The
    labels are kept within LABEL px of symmetric transfer distance 0.5 (d0 + d1), so each forward distance d0 is below 2 LABEL < 3 px:
    every label is correct at 3 px.  The homography estimated from them lies within LABEL px at the corners."""
    from openglue_amd import features, pairs, supervision, synthetic as syn
    from openglue_amd.sift import SIFT
    dev = gpu_device
    LABEL = 1.0
    rgb = torch.stack([torch.cat([syn.make_image(240, 320, seed=51 + 3 * b + c)[0] for c in range(3)]) for b in range(2)])
    frames = (rgb * 255).round().to(torch.uint8).permute(0, 2, 3, 1).contiguous().to(dev)
    wo = torch.tensor([[[10, -7], [-12, 9], [-5, -20], [14, 6]], [[-16, 4], [8, 12], [20, -3], [-6, -18]]], dtype=torch.float32, device=dev)
    item = pairs.homography_pairs(frames, 24, wo)
    net = SIFT(max_keypoints=512)
    f = [features.prepare_features_output(*net(item[k]), "none") for k in ("image0", "image1")]
    _, y = supervision.generate_gt_matches(item, f[0], f[1], LABEL, LABEL, apply_thresholds=True)
    gt = y["gt_matches0"]
    matched = (gt >= 0).sum(1)
    assert int(matched.min()) >= 20, matched.tolist()
    h, w = item["image0"].shape[2:]
    acc = metrics.HomographyAccuracy(3.0)
    acc.update_batch(f[0]["keypoints"], f[1]["keypoints"], gt, item["transformation"])
    got = acc.compute()
    assert float(got["Precision"]) == 1.0 and 0 < float(got["Matching Score"]) <= 1.0
    r = geometry.homography(f[0]["keypoints"], f[1]["keypoints"], gt, hypotheses=256)
    err = metrics.homography_error(r["H"], item["transformation"]["H"], (w, h)).cpu()
    parity_note(f"homography, end to end: labels {matched.tolist()}, inliers {r['num_inliers'].tolist()}, corner error "
                f"{[round(float(v), 3) for v in err]} px at {w} x {h}")
    assert bool((err < LABEL).all()), err.tolist()
    for b in range(2):
        band_check(r["H"][b].cpu(), f[0]["keypoints"][b].cpu(), f[1]["keypoints"][b].cpu(), gt[b].cpu(), r["inliers"][b].cpu(),
                   label=f"homography, end to end pair {b}")
