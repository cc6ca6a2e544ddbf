"""Uncalibrated geometric verification on the MI355X (openglue_amd.geometry, csrc/geometry.hip) against the float64 restatement
(tests/geometry_ref.py): the seven-point solver on exact minimal problems, RANSAC on noise-free and noisy scenes, the edges, the
consistency of the mask with the returned F, the refit, determinism and batching, and the path from labels / SuperGlue.match."""
import functools

import numpy as np
import pytest
import torch

from openglue_amd import geometry
from tests import geometry_ref as ref
from tests import metrics_ref
from tests.util import parity_note

pytestmark = pytest.mark.gpu

THR = 1.0          # pixels


def run(k0, k1, m0, dev, nk=None, **kw):
    r = geometry.fundamental_matrix(k0.to(dev), k1.to(dev), m0.to(dev), None if nk is None else nk.to(dev), **kw)
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in r.items()}


def scenes(specs, **kw):
    """One pair per (outliers, seed) -> a batch."""
    parts = [ref.make_scene(1, outliers=o, seed=s, **kw) for o, s in specs]
    tr = {k: torch.cat([p[3][k] for p in parts]) for k in parts[0][3]}
    return torch.cat([p[0] for p in parts]), torch.cat([p[1] for p in parts]), torch.cat([p[2] for p in parts]), tr, torch.cat([p[4] for p in parts])


def seed_with_clean_samples(clean, hypotheses, pair_offset=0):
    """The first RANSAC seed under which every pair draws at least one all-inlier sample.  clean: per pair, the truth (True =
    inlier) over the pair's valid matches in index order.  Decided from the restatement's draws alone, before any kernel runs: a
    fixed number of hypotheses finds the scene only if one of them is clean (0.4^7 x 512 is below one expected sample)."""
    for seed in range(200):
        if all(any(all(c[r] for r in ref.draw_distinct(seed, pair_offset + b, h, len(c))) for h in range(hypotheses)) for b, c in enumerate(clean)):
            return seed
    raise AssertionError("no seed below 200 draws a clean sample for every pair")


def band_check(F, k0, k1, m0, inliers, nk=None, thr=THR, label=None):
    """Rule 4: with the returned F in float64, a valid match with d^2 < 0.99 thr^2 is flagged, one with d^2 > 1.01 thr^2 is not, and
    nothing else is flagged.  Returns (matches in between, valid matches, d^2 of the valid matches, their index); with `label` the
    number in between goes to the parity notes."""
    idx, p0, p1 = ref.valid_matches(k0.numpy(), k1.numpy(), m0.numpy(), nk)
    inl = inliers.numpy()
    other = np.ones(len(inl), dtype=bool)
    other[idx] = False
    assert not inl[other].any(), "a keypoint without a valid match is flagged"
    d2 = ref.sampson_sq(F.numpy(), p0, p1)
    t2 = thr * thr
    assert inl[idx][d2 < 0.99 * t2].all(), int((~inl[idx][d2 < 0.99 * t2]).sum())
    assert not inl[idx][d2 > 1.01 * t2].any(), int(inl[idx][d2 > 1.01 * t2].sum())
    between = int(((d2 >= 0.99 * t2) & (d2 <= 1.01 * t2)).sum())
    if label:
        parity_note(f"{label}: {between} of {len(idx)} matches within 1 % of the threshold^2")
    assert between <= 0.02 * max(len(idx), 1), (between, len(idx))
    return between, len(idx), d2, idx


def unit_and_signed(F):
    F = F.numpy()
    return abs(np.linalg.norm(F) - 1) < 1e-12 and F.reshape(9)[np.abs(F).argmax()] > 0


# ------------------------------------------------------------------------------------------------ 1. minimal solver
def test_seven_point_solver(gpu_device):
    P = 2049
    k0, k1, _, tr, _ = ref.make_scene(P, 7, seed=3, dtype=torch.float64)
    x0, x1, Ft = np.zeros((P, 7, 2)), np.zeros((P, 7, 2)), np.zeros((P, 3, 3))
    for p in range(P):
        (c0, s0), (c1, s1) = ref.hartley(k0[p].numpy()), ref.hartley(k1[p].numpy())
        T0 = np.array([[s0, 0, -s0 * c0[0]], [0, s0, -s0 * c0[1]], [0, 0, 1.0]])
        T1 = np.array([[s1, 0, -s1 * c1[0]], [0, s1, -s1 * c1[1]], [0, 0, 1.0]])
        x0[p], x1[p] = (k0[p].numpy() - c0) * s0, (k1[p].numpy() - c1) * s1
        f = np.linalg.inv(T1).T @ tr["F"][p].numpy() @ np.linalg.inv(T0)
        Ft[p] = f / np.linalg.norm(f)
    F, ns = geometry.fundamental_7pt(torch.from_numpy(x0).to(gpu_device), torch.from_numpy(x1).to(gpu_device))
    torch.cuda.synchronize()
    F, ns = F.cpu().numpy(), ns.cpu().numpy()
    assert np.isfinite(F).all() and ns.min() >= 0 and ns.max() <= 3
    err = lambda sols, t: min([min(np.abs(f - t).max(), np.abs(f + t).max()) for f in sols] or [np.inf])
    near, worst = 0, 0.0
    for p in range(P):
        A = ref.constraint_rows(x0[p], x1[p])
        for s in range(ns[p]):
            f = F[p, s]
            assert abs(np.linalg.norm(f) - 1) < 1e-9
            assert abs(np.linalg.det(f)) <= 1e-9 and np.abs(A @ f.reshape(9)).max() <= 1e-9, (p, s)
        assert not F[p, ns[p]:].any(), p                      # the unused slots are zero
        sols, nd = ref.seven_point(x0[p], x1[p])
        e_ref, e_gpu = err(sols, Ft[p]), err(list(F[p, :ns[p]]), Ft[p])
        worst = max(worst, e_gpu)
        assert e_gpu <= max(10 * e_ref, 1e-9), (p, e_gpu, e_ref)
        near += nd
        if not nd:
            assert ns[p] == len(sols), (p, ns[p], len(sols))
    parity_note(f"seven-point solver: {P} problems, mean {ns.mean():.2f} solutions, worst error of the true F {worst:.2e}, "
                f"{near} near-double cubics left out of the count comparison")
    assert near <= 0.01 * P
    # two identical correspondences: rank 6, any answer but a finite one
    x0[0, 1], x1[0, 1] = x0[0, 0], x1[0, 0]
    Fd, nd = geometry.fundamental_7pt(torch.from_numpy(x0[:1]).to(gpu_device), torch.from_numpy(x1[:1]).to(gpu_device))
    assert bool(torch.isfinite(Fd).all()) and 0 <= int(nd[0]) <= 3


# ------------------------------------------------------------------------------------------------ 2. noise-free RANSAC
def test_ransac_noise_free(gpu_device):
    k0, k1, m0, tr, out = scenes([(0.0, 10), (0.3, 11), (0.6, 12), (0.3, 13)], n=300)
    B, H = 4, 512
    seed = seed_with_clean_samples([(~out[b]).tolist() for b in range(B)], H)
    r = run(k0, k1, m0, gpu_device, hypotheses=H, seed=seed)
    for b in range(B):
        assert torch.equal(r["inliers"][b], ~out[b]), (b, int((r["inliers"][b] != ~out[b]).sum()))
        assert int(r["num_inliers"][b]) == int((~out[b]).sum()) and int(r["best_model"][b]) >= 0
        assert unit_and_signed(r["F"][b])
        band_check(r["F"][b], k0[b], k1[b], m0[b], r["inliers"][b], label=f"noise-free RANSAC pair {b}")
        want = ref.fundamental_matrix(k0[b].numpy(), k1[b].numpy(), m0[b].numpy(), hypotheses=H, seed=seed, pair=b)
        assert want["best_model"] // 3 == int(r["best_model"][b]) // 3, (b, want["best_model"], int(r["best_model"][b]))
        good = (~out[b]).numpy()
        d_gpu = np.sqrt(ref.sampson_sq(r["F"][b].numpy(), k0[b].double().numpy()[good], k1[b].double().numpy()[good]).max())
        d_ref = np.sqrt(ref.sampson_sq(want["F"], k0[b].double().numpy()[good], k1[b].double().numpy()[good]).max())
        parity_note(f"noise-free RANSAC pair {b}: largest Sampson distance of the true matches {d_gpu:.2e} px (restatement {d_ref:.2e})")
        assert d_gpu <= 4 * d_ref, (b, d_gpu, d_ref)


# ------------------------------------------------------------------------------------------------ 3. edges
def test_edges_small(gpu_device):
    """M = 70 rows (fewer than a workgroup has threads), N = 64: no match, 6 matches, exactly 7, pure chance, ragged with holes and
    entries >= N, every point on one spot.  refine = 2, 86 hypotheses (258 models: not a multiple of 256), then the chance pair with
    8 hypotheses (a winner of 7 inliers among 12 matches: no refit), then a single hypothesis."""
    M, N = 70, 64
    k0, k1, _, tr, _ = ref.make_scene(6, M, seed=60)
    k1 = k1[:, :N]
    g = torch.Generator().manual_seed(61)
    m0 = torch.arange(M).repeat(6, 1)
    m0[m0 >= N] = 1000                                        # entries >= N are no matches
    m0[0] = -1
    m0[1, 6:] = -1
    m0[2, :20] = -1
    m0[2, 27:] = -1                                           # exactly 7
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
        assert not bool(a["F"][b].any())
    assert int(a["num_inliers"][2]) == 7 and bool(a["inliers"][2, 20:27].all()) and int(a["inliers"][2].sum()) == 7
    assert all(torch.equal(a[k][2], a0[k][2]) for k in a)     # exactly 7 matches: nothing to refit
    for b in (2, 3):
        assert 7 <= int(a["num_inliers"][b]) and 0 <= int(a["best_model"][b]) < 3 * 86 and unit_and_signed(a["F"][b])
    assert int(a0["num_inliers"][2]) == 7
    for b in range(6):
        assert int(a["num_inliers"][b]) == int(a["inliers"][b].sum())
        assert int(a["num_inliers"][b]) >= int(a0["num_inliers"][b])
        band_check(a["F"][b], k0[b], k1[b], m0[b], a["inliers"][b], int(nk[b]))
    # pair 3 again with 8 hypotheses: 12 valid matches, and by the restatement no model holds more than its own 7 (the eighth match
    # lies tens of pixels off the winner's lines), so the winner has fewer than 8 inliers and both refit rounds are skipped
    want = ref.fundamental_matrix(k0[3].numpy(), k1[3].numpy(), m0[3].numpy(), hypotheses=8, refine=0, pair=3)
    assert want["ransac_inliers"] == 7
    c2 = run(k0[3:4], k1[3:4], m0[3:4], gpu_device, hypotheses=8, refine=2, pair_offset=3)
    c0 = run(k0[3:4], k1[3:4], m0[3:4], gpu_device, hypotheses=8, refine=0, pair_offset=3)
    assert int(c0["num_inliers"][0]) == 7 and int(c0["best_model"][0]) == want["best_model"]
    assert all(torch.equal(c2[k], c0[k]) for k in c2) and unit_and_signed(c2["F"][0])
    band_check(c2["F"][0], k0[3], k1[3], m0[3], c2["inliers"][0])
    # pair 4: noise-free matches among the holes; its valid ones are all inliers once a sample is clean
    idx4, _, _ = ref.valid_matches(k0[4].numpy(), k1[4].numpy(), m0[4].numpy(), 68)
    assert 7 < len(idx4) < 64 and int(a["num_inliers"][4]) == len(idx4)
    # one hypothesis: on a noise-free pair without outliers the one sample is clean
    one = run(k0[4:5], k1[4:5], m0[4:5], gpu_device, nk=nk[4:5], hypotheses=1)
    assert int(one["best_model"][0]) in (0, 1, 2) and int(one["num_inliers"][0]) == len(idx4)
    assert torch.equal(torch.nonzero(one["inliers"][0])[:, 0], torch.from_numpy(idx4))


def test_edges_more_matches_than_one_chunk(gpu_device):
    """M = 1100 with more than 1024 valid matches: the scorer stages its points in two chunks."""
    k0, k1, m0, tr, out = ref.make_scene(2, 1100, outliers=0.3, seed=62)
    m0[1, 5] = -1
    clean = [(~out[0]).tolist(), [bool(v) for i, v in enumerate((~out[1]).tolist()) if i != 5]]
    seed = seed_with_clean_samples(clean, 86)
    r = run(k0, k1, m0, gpu_device, hypotheses=86, seed=seed)
    for b in range(2):
        want = ~out[b]
        if b == 1:
            want[5] = False
        assert torch.equal(r["inliers"][b], want), (b, int((r["inliers"][b] != want).sum()))
        assert int(r["num_inliers"][b]) == int(want.sum())
        band_check(r["F"][b], k0[b], k1[b], m0[b], r["inliers"][b])


def test_edges_more_pairs_than_a_grid_is_high(gpu_device):
    """65540 pairs of 8 noise-free matches, one hypothesis: the pair index runs along the grid's x extent, which has room for it
    (y ends at 65535).  Every sample is clean, so every pair keeps its 8 matches, and the last pair equals a call of its own."""
    k0, k1, m0, _, _ = ref.make_scene(4, 8, seed=63)
    B = 65540
    K0, K1, M0 = k0.repeat(B // 4, 1, 1), k1.repeat(B // 4, 1, 1), m0.repeat(B // 4, 1)
    r = run(K0, K1, M0, gpu_device, hypotheses=1)
    assert bool((r["num_inliers"] == 8).all()) and bool(r["inliers"].all()) and bool((r["best_model"] >= 0).all())
    assert bool(torch.isfinite(r["F"]).all())
    one = run(K0[-1:], K1[-1:], M0[-1:], gpu_device, hypotheses=1, pair_offset=B - 1)
    for k in r:
        assert torch.equal(one[k][0], r[k][B - 1]), k
    band_check(r["F"][B - 1], K0[-1], K1[-1], M0[-1], r["inliers"][B - 1])


# ------------------------------------------------------------------------------------------------ 5, 6. noisy scenes
NOISY_H = 256


@functools.lru_cache(maxsize=None)
def noisy():
    """Four pairs of 300 matches and one of 1100, 0.5 px noise, 30 % outliers, with the restatement's results at refine 0 and 2
    and the inlier count of the true F.  Computed once, read by both tests."""
    small = ref.make_scene(4, 300, outliers=0.3, noise=0.5, seed=70)
    big = ref.make_scene(1, 1100, outliers=0.3, noise=0.5, seed=71)
    res = []
    for (k0, k1, m0, tr, _), offset in ((small, 0), (big, 0)):
        for b in range(k0.shape[0]):
            a = (k0[b].numpy(), k1[b].numpy(), m0[b].numpy())
            r0 = ref.fundamental_matrix(*a, hypotheses=NOISY_H, refine=0, pair=offset + b)
            r2 = ref.fundamental_matrix(*a, hypotheses=NOISY_H, refine=2, pair=offset + b)
            true = int((ref.sampson_sq(tr["F"][b].numpy(), k0[b].double().numpy(), k1[b].double().numpy()) <= THR * THR).sum())
            res.append((r0, r2, true))
    return small, big, res


def test_winner_against_restatement(gpu_device):
    (k0, k1, m0, tr, _), _, res = noisy()
    r = run(k0, k1, m0, gpu_device, hypotheses=NOISY_H, refine=0)
    for b in range(4):
        between, n, d2, _ = band_check(r["F"][b], k0[b], k1[b], m0[b], r["inliers"][b])
        c = int((d2 <= THR * THR).sum())
        d2_ref = ref.sampson_sq(res[b][0]["F"], k0[b].double().numpy(), k1[b].double().numpy())
        band = lambda d: (d >= 0.99 * THR * THR) & (d <= 1.01 * THR * THR)
        k = int((band(d2) | band(d2_ref)).sum())
        c_ref = res[b][0]["ransac_inliers"]
        parity_note(f"RANSAC winner pair {b}: fp64 inliers of the returned F {c}, restatement {c_ref}, {k} matches in the 1 % band "
                    f"({between} under the returned F), models {int(r['best_model'][b])} / {res[b][0]['best_model']}")
        assert c >= c_ref - k, (b, c, c_ref, k)
        assert int(r["num_inliers"][b]) == int(r["inliers"][b].sum())


def test_refit(gpu_device):
    small, big, res = noisy()
    worst_gpu, worst_ref, worst_min = 2.0, 2.0, 2.0
    for (k0, k1, m0, tr, _), first in ((small, 0), (big, 4)):
        r0 = run(k0, k1, m0, gpu_device, hypotheses=NOISY_H, refine=0)
        r2 = run(k0, k1, m0, gpu_device, hypotheses=NOISY_H, refine=2)
        assert torch.equal(r0["best_model"], r2["best_model"])
        for b in range(k0.shape[0]):
            n0, n2 = int(r0["num_inliers"][b]), int(r2["num_inliers"][b])
            assert n2 >= n0, (first + b, n2, n0)
            band_check(r2["F"][b], k0[b], k1[b], m0[b], r2["inliers"][b], label=f"refit pair {first + b}")
            assert unit_and_signed(r2["F"][b]) and n2 == int(r2["inliers"][b].sum())
            _, ref2, true = res[first + b]
            ratio, ratio_ref = n2 / true, ref2["num_inliers"] / true
            worst_gpu, worst_ref, worst_min = min(worst_gpu, ratio), min(worst_ref, ratio_ref), min(worst_min, n0 / true)
            parity_note(f"refit pair {first + b}: inliers / true-F inliers {n0 / true:.3f} -> {ratio:.3f} (restatement {ratio_ref:.3f})")
            assert ratio >= ratio_ref - 0.02, (first + b, ratio, ratio_ref)
    parity_note(f"refit, 0.5 px noise, 30 % outliers, {NOISY_H} hypotheses: worst inliers / true-F inliers {worst_min:.3f} (minimal model) -> "
                f"{worst_gpu:.3f} (two refits), restatement {worst_ref:.3f}")


# ------------------------------------------------------------------------------------------------ 7. determinism and batching
def test_deterministic_and_batched_equals_per_pair(gpu_device):
    B, M = 4, 300
    k0, k1, m0, tr, _ = ref.make_scene(B, M, outliers=0.3, noise=0.5, seed=80)
    g = torch.Generator().manual_seed(81)
    m0[torch.rand(B, M, generator=g) < 0.3] = -1
    m0[2, 3:] = -1                                     # too few matches for a model
    nk = torch.randint(M // 2, M + 1, (B,), generator=g, dtype=torch.int32)
    kw = dict(hypotheses=200, seed=9)
    a = run(k0, k1, m0, gpu_device, nk=nk, **kw)
    b2 = run(k0, k1, m0, gpu_device, nk=nk, **kw)
    for k in a:
        assert torch.equal(a[k], b2[k]), k
    assert int(a["best_model"][2]) == -1 and int(a["best_model"][0]) >= 0
    for b in range(B):
        one = run(k0[b:b + 1], k1[b:b + 1], m0[b:b + 1], gpu_device, nk=nk[b:b + 1], pair_offset=b, **kw)
        for k in a:
            assert torch.equal(one[k][0], a[k][b]), (b, k)
        keep = (m0[b] >= 0) & (torch.arange(M) < int(nk[b]))
        F, inl = geometry.find_fundamental(k0[b][keep].to(gpu_device), k1[b][m0[b][keep]].to(gpu_device), pair_offset=b, **kw)
        assert torch.equal(F.cpu(), a["F"][b]), b
        assert torch.equal(inl.cpu(), a["inliers"][b][keep]), b
        band_check(a["F"][b], k0[b], k1[b], m0[b], a["inliers"][b], int(nk[b]), label=f"batched pair {b}")


# ------------------------------------------------------------------------------------------------ 8. end to end
def test_end_to_end_from_labels_and_match(gpu_device):
    from openglue_amd import supervision, synthetic as syn
    from openglue_amd.superglue import SuperGlue
    dev = gpu_device
    B, n = 4, 512
    k0, k1, _, tr, _ = ref.make_scene(B, n, seed=50)
    # depths of every keypoint in both cameras (exact scene): labels by reprojection
    d0, d1 = [], []
    for b in range(B):
        x0 = metrics_ref.normalize_with_intrinsics(k0[b], tr["K0"][b])
        x1 = metrics_ref.normalize_with_intrinsics(k1[b], tr["K1"][b])
        h0 = torch.cat([x0, torch.ones(n, 1, dtype=torch.float64)], 1)
        h1 = torch.cat([x1, torch.ones(n, 1, dtype=torch.float64)], 1)
        a = torch.linalg.cross(h1, h0 @ tr["R"][b].T)
        c = torch.linalg.cross(h1, tr["T"][b].expand(n, 3))
        z0 = -(a * c).sum(1) / (a * a).sum(1)
        d0.append(z0)
        d1.append((h0 * z0[:, None] @ tr["R"][b].T + tr["T"][b])[:, 2])
    trl = {**{k: tr[k].float().to(dev) for k in ("K0", "K1", "R", "T")}, "type": ["3d_reprojection"] * B,
           "depth0": torch.stack(d0).float().to(dev), "depth1": torch.stack(d1).float().to(dev)}
    feats = lambda k: {"keypoints": k.to(dev), "local_descriptors": torch.zeros(B, n, 4, device=dev), "side_info": torch.zeros(B, n, 1, device=dev)}
    _, y = supervision.generate_gt_matches({"transformation": trl}, feats(k0), feats(k1), 3.0, 5.0)
    gt = y["gt_matches0"].cpu()
    r = geometry.fundamental_matrix(k0.to(dev), k1.to(dev), y["gt_matches0"], hypotheses=64)
    r = {k: v.cpu() for k, v in r.items()}
    for b in range(B):
        band_check(r["F"][b], k0[b], k1[b], gt[b], r["inliers"][b], label=f"end to end, labels, pair {b}")
        # the true geometry: every label lies on its epipolar line, so the true F and the returned one flag the same matches
        band_check(tr["F"][b], k0[b], k1[b], gt[b], r["inliers"][b])
        assert int(r["num_inliers"][b]) == int(((gt[b] >= 0) & (gt[b] < n)).sum()) >= 8
    # SuperGlue.match output goes straight in
    cfg = syn.make_config(descriptor_dim=64, num_stages=2, num_heads=4, num_iters=3, side_info_size=1)
    model = SuperGlue(cfg).eval()
    model.load_state_dict(syn.make_state_dict(cfg, seed=0), strict=True)
    model.to(dev)
    data = syn.make_batch(2, 64, 80, 64, 1, seed=123)
    out = model.match({k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in data.items()}, 0.2)
    m = geometry.fundamental_matrix(data["keypoints0"].to(dev), data["keypoints1"].to(dev), out["matches0"], hypotheses=64)
    torch.cuda.synchronize()
    for b in range(2):
        assert bool(torch.isfinite(m["F"][b]).all())
        band_check(m["F"][b].cpu(), data["keypoints0"][b], data["keypoints1"][b], out["matches0"][b].cpu(), m["inliers"][b].cpu(),
                   label=f"end to end, SuperGlue.match, pair {b}")
