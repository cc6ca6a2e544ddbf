"""Seeded inputs for the tests of the training criterion (openglue_amd.supervision.criterion, csrc/supervision.hip), and a float64
census of which of its branches a case takes.  Plain torch on the CPU; tests/test_supervision_cpu.py, tests/test_gpu_criterion.py
and tests/golden/make_golden_criterion.py all build their inputs here, so the fixture stores results only.

Independent Gaussian descriptors put every half-cosine distance near 0.5: with margin 0.2 every matched triplet fires and no
unmatched hinge does.  `crit_case` spreads the distances instead: positives from d_ap ~ 0 to ~ 0.5, a third of the unmatched
keypoints with a close neighbour, ignored labels on both sides, column norms from 0.1 to 10, and per batch entry a pair that is
half matched, one with an image fully matched, and (B > 1) one without any match.
"""
from __future__ import annotations

import torch

from oracle.superglue_oracle import pairwise_cosine_dist
from tests import supervision_ref as ref

MARGIN = 0.2
W_LOSS, W_METRIC = 0.7, 1.9          # upstream weights of the backward pass: (W_LOSS * loss + W_METRIC * metric_loss).backward()
MIN_HINGE, MIN_GAP = 5e-4, 2e-5      # floors of the census; the fp32 distances differ from float64 by < 4e-7
FAMILIES = ("triplet01", "triplet10", "unmatched0", "unmatched1")

# (B, m, n, D) -> seed: the first seed whose census meets `regular_case_ok`
REGULAR = {
    (2, 70, 90, 128): 0,      # the shape of supervision.npz's crit_d128, with mixed hinges
    (1, 64, 64, 32): 0,       # exactly one whole Gram tile, D = one k slab, D < 64 lanes
    (3, 65, 63, 64): 0,       # one past and one short of a tile edge; pair 1 has image 1 fully matched
    (2, 130, 200, 40): 2,     # 3 x 4 tiles, D not a multiple of the k slab
    (1, 300, 520, 64): 1,     # the 256-thread strided loops of pair_loss_kernel
    (2, 5, 3, 8): 0,          # less than a half-wave
    (4, 33, 31, 256): 0,      # B = 4
}
SMALL = (2, 5, 3, 8)                 # too few terms for every family to have both an active and an inactive one
SINGLE = ((1, 7), (7, 1), (1, 1))    # (m, n) of the cases whose positive is the only entry of its row / column
ZERO_SHAPE = (1, 64, 64, 32)
TIE_SHAPE = (1, 70, 150, 64)
TIE_SEED = 0


def case_name(shape) -> str:
    return "b%d_m%d_n%d_d%d" % tuple(shape)


def crit_case(B, m, n, D, seed):
    """-> (scores [B, m+1, n+1] log-probabilities, desc0 [B, D, m], desc1 [B, D, n], gt0 [B, m], gt1 [B, n]) in fp32 / int64."""
    g = torch.Generator().manual_seed(seed)
    A = torch.randn(B, D, m, generator=g, dtype=torch.float64)
    Bd = torch.randn(B, D, n, generator=g, dtype=torch.float64)
    gt0 = torch.full((B, m), -1, dtype=torch.long)
    gt1 = torch.full((B, n), -1, dtype=torch.long)
    for b in range(B):
        # nothing matched / half / one image fully matched
        k = 0 if (B > 1 and b == B - 1) else (min(m, n) // 2 if b == 0 else min(m, n))
        i = torch.randperm(m, generator=g)[:k]
        j = torch.randperm(n, generator=g)[:k]
        gt0[b, i] = j
        gt1[b, j] = i
        sig = torch.logspace(-1.5, 0.7, max(k, 1), dtype=torch.float64)[:k]               # d_ap from ~0 to ~0.5
        Bd[b][:, j] = A[b][:, i] + sig * torch.randn(D, k, generator=g, dtype=torch.float64)
        u0 = (gt0[b] == -1).nonzero()[:, 0]
        u1 = (gt1[b] == -1).nonzero()[:, 0]
        p = min(len(u0), len(u1)) // 3                                                    # a third of the unmatched get a close neighbour
        if p:
            Bd[b][:, u1[:p]] = A[b][:, u0[:p]] + 0.5 * torch.randn(D, p, generator=g, dtype=torch.float64)
        if len(u0) > p:
            gt0[b, u0[p:p + max(1, len(u0) // 10)]] = -2                                  # ignored labels on both sides
        if len(u1) > p:
            gt1[b, u1[p:p + max(1, len(u1) // 10)]] = -2
    A = A * 10 ** (torch.rand(B, 1, m, generator=g, dtype=torch.float64) * 2 - 1)         # column norms 0.1 .. 10
    Bd = Bd * 10 ** (torch.rand(B, 1, n, generator=g, dtype=torch.float64) * 2 - 1)
    S = torch.log_softmax(torch.randn(B, (m + 1) * (n + 1), generator=g, dtype=torch.float64), -1).reshape(B, m + 1, n + 1)
    return S.float(), A.float(), Bd.float(), gt0, gt1


def regular_case(shape):
    return crit_case(*shape, REGULAR[tuple(shape)])


def single_case(m, n, D=64, seed=0):
    """B = 1 with one match whose positive is the only entry of its row (n == 1) and / or column (m == 1): the reference masks
    it with +inf, argmin of the all-inf line is 0, d_an is gathered from the unmasked distances, so d_an == d_ap and the
    triplet term is exactly the margin, without gradient.  Every other keypoint is unmatched."""
    g = torch.Generator().manual_seed(1000 * m + n + seed)
    A = torch.randn(1, D, m, generator=g, dtype=torch.float64)
    Bd = torch.randn(1, D, n, generator=g, dtype=torch.float64)
    i, j = (m - 1) // 2, (n - 1) // 2                       # (1, 7): gt0 = [[3]]
    gt0 = torch.full((1, m), -1, dtype=torch.long)
    gt1 = torch.full((1, n), -1, dtype=torch.long)
    gt0[0, i], gt1[0, j] = j, i
    Bd[0][:, j] = A[0][:, i] + 0.8 * torch.randn(D, generator=g, dtype=torch.float64)
    if n > 1:                                               # one unmatched keypoint within the margin of the other image
        Bd[0][:, (j + 1) % n] = A[0][:, i] + 0.5 * torch.randn(D, generator=g, dtype=torch.float64)
    if m > 1:
        A[0][:, (i + 1) % m] = Bd[0][:, j] + 0.5 * torch.randn(D, generator=g, dtype=torch.float64)
    S = torch.log_softmax(torch.randn(1, (m + 1) * (n + 1), generator=g, dtype=torch.float64), -1).reshape(1, m + 1, n + 1)
    return S.float(), A.float(), Bd.float(), gt0, gt1


def zero_case():
    """The one-tile case with one unmatched column of desc0 and one matched column of desc1 set to exactly 0.  F.normalize
    clamps them to a^ = 0: their distance to a unit vector is 0.25 (not 0.5 (1 - cos) = 0.5) and to each other 0.
    -> (scores, desc0, desc1, gt0, gt1, i_zero, j_zero)"""
    S, A, Bd, gt0, gt1 = regular_case(ZERO_SHAPE)
    iz = int((gt0[0] == -1).nonzero()[0, 0])
    jz = int((gt1[0] >= 0).nonzero()[0, 0])
    A[0, :, iz] = 0.0
    Bd[0, :, jz] = 0.0
    return S, A, Bd, gt0, gt1, iz, jz


def tie_case(ignore_copies=False):
    """Exact ties across a Gram tile edge.  After the scaling step column `hi` of desc1 becomes a bit-identical copy of column
    `lo` (lo < 64 <= hi, both unmatched), built to be the closest neighbour of the unmatched keypoint u and the hardest negative
    of the matched keypoint r of image 0; mirrored, rows lo2 < 64 <= hi2 of desc0 for the unmatched v and the matched c of
    image 1.  All four argmins then see a tie between two workgroups, and the lower index has to win as in torch.argmin.
    `ignore_copies` labels the two higher-index copies -2, which removes their own hinge: their gradient is then exactly 0.
    -> (scores, desc0, desc1, gt0, gt1, info)"""
    S, A, Bd, gt0, gt1 = crit_case(*TIE_SHAPE, TIE_SEED)
    g = torch.Generator().manual_seed(TIE_SEED + 77)
    D = A.shape[1]
    un0, un1 = (gt0[0] == -1).nonzero()[:, 0].tolist(), (gt1[0] == -1).nonzero()[:, 0].tolist()
    ma0 = (gt0[0] >= 0).nonzero()[:, 0].tolist()
    lo, hi = [j for j in un1 if j < 64][0], [j for j in un1 if j >= 64][0]
    lo2, hi2 = [i for i in un0 if i < 64][0], [i for i in un0 if i >= 64][0]
    dist = pairwise_cosine_dist(A.double().transpose(2, 1).contiguous(), Bd.double().transpose(2, 1).contiguous())[0]
    far0, far1 = dist.amin(1) > 0.3, dist.amin(0) > 0.3       # u and v: unmatched keypoints without a close neighbour so far
    u = [i for i in un0 if i not in (lo2, hi2) and far0[i]][0]
    r = ma0[0]
    v = [j for j in un1 if j not in (lo, hi) and far1[j]][0]
    c = [int(gt0[0, i]) for i in ma0 if i != r][0]
    unit = lambda x: x / x.norm()
    Bd[0, :, lo] = 3.0 * (unit(A[0, :, u]) + unit(A[0, :, r]) + 0.2 * unit(torch.randn(D, generator=g)))
    Bd[0, :, hi] = Bd[0, :, lo]
    A[0, :, lo2] = 0.3 * (unit(Bd[0, :, v]) + unit(Bd[0, :, c]) + 0.2 * unit(torch.randn(D, generator=g)))
    A[0, :, hi2] = A[0, :, lo2]
    if ignore_copies:
        gt1[0, hi] = -2
        gt0[0, hi2] = -2
    return S, A, Bd, gt0, gt1, dict(lo=lo, hi=hi, lo2=lo2, hi2=hi2, u=u, r=r, v=v, c=c)


def _best_two(d, dim):
    """(argmin, second-best minus best) along `dim`; the gap is +inf where fewer than two candidates are finite."""
    idx = torch.argmin(d, dim=dim)
    if d.shape[dim] < 2:
        return idx, torch.full(idx.shape, float("inf"), dtype=d.dtype)
    two = d.topk(2, dim=dim, largest=False).values
    first, second = two.select(dim, 0), two.select(dim, 1)
    gap = torch.where(torch.isfinite(second), second - first, torch.full_like(first, float("inf")))
    return idx, gap


def census(desc0, desc1, gt0, gt1, margin=MARGIN):
    """Which branches of the metric loss a case takes, in float64:
      counts[family]  (active, inactive) hinge terms of triplet01 / triplet10 / unmatched0 / unmatched1
      min_hinge       the smallest |hinge argument|
      min_gap         the smallest gap between the best and the second-best candidate of any argmin the loss uses
      gaps[family]    every such gap (a tie between bit-identical descriptors is exactly 0)
      args[family]    every hinge argument
      winners[family] [k, 3] int64 rows (pair, anchor keypoint, chosen keypoint of the other image) behind those gaps
    """
    dist = pairwise_cosine_dist(desc0.double().transpose(2, 1).contiguous(), desc1.double().transpose(2, 1).contiguous())
    b, i0 = torch.where(gt0 >= 0)
    i1 = gt0[b, i0]
    dd = dist.clone()
    dd[b, i0, i1] = float("inf")
    rowm, rowm_gap = _best_two(dd, 2)
    colm, colm_gap = _best_two(dd, 1)
    row, row_gap = _best_two(dist, 2)
    col, col_gap = _best_two(dist, 1)
    d_ap = dist[b, i0, i1]
    args = {"triplet01": d_ap - dist[b, i0, rowm[b, i0]] + margin, "triplet10": d_ap - dist[b, colm[b, i1], i1] + margin}
    gaps = {"triplet01": rowm_gap[b, i0], "triplet10": colm_gap[b, i1]}
    winners = {"triplet01": torch.stack([b, i0, rowm[b, i0]], 1), "triplet10": torch.stack([b, i1, colm[b, i1]], 1)}
    b0, u0 = torch.where(gt0 == -1)
    args["unmatched0"] = margin - dist[b0, u0, row[b0, u0]]
    gaps["unmatched0"] = row_gap[b0, u0]
    winners["unmatched0"] = torch.stack([b0, u0, row[b0, u0]], 1)
    b1, u1 = torch.where(gt1 == -1)
    args["unmatched1"] = margin - dist[b1, col[b1, u1], u1]
    gaps["unmatched1"] = col_gap[b1, u1]
    winners["unmatched1"] = torch.stack([b1, u1, col[b1, u1]], 1)
    counts = {f: (int((args[f] > 0).sum()), int((args[f] <= 0).sum())) for f in FAMILIES}
    every_arg = torch.cat([args[f] for f in FAMILIES])
    every_gap = torch.cat([gaps[f] for f in FAMILIES])
    return dict(counts=counts, args=args, gaps=gaps, winners=winners,
                min_hinge=float(every_arg.abs().min()) if every_arg.numel() else float("inf"),
                min_gap=float(every_gap.min()) if every_gap.numel() else float("inf"))


def regular_case_ok(shape, cen) -> list:
    """The conditions a regular case has to meet, as a list of the ones it misses (empty: fine)."""
    missed = []
    if tuple(shape) != SMALL:
        missed += [f"{f}: active / inactive {cen['counts'][f]}" for f in FAMILIES if min(cen["counts"][f]) < 1]
    if not cen["min_hinge"] >= MIN_HINGE:
        missed.append(f"min |hinge argument| {cen['min_hinge']:.3g} < {MIN_HINGE}")
    if not cen["min_gap"] >= MIN_GAP:
        missed.append(f"min argmin gap {cen['min_gap']:.3g} < {MIN_GAP}")
    return missed


def tie_case_ok(case):
    """Preconditions of `tie_case`: every one of the four argmin families has an exact tie that the lower-index copy wins, at least once
    on an active hinge term; every other gap and every hinge argument clears the floors."""
    _, A, Bd, gt0, gt1, info = case
    lo, hi, lo2, hi2 = (info[k] for k in ("lo", "hi", "lo2", "hi2"))
    assert lo < 64 <= hi and lo2 < 64 <= hi2
    assert torch.equal(Bd[0, :, lo], Bd[0, :, hi]) and torch.equal(A[0, :, lo2], A[0, :, hi2])
    assert gt1[0, lo] == -1 and gt0[0, lo2] == -1 and gt1[0, hi] in (-1, -2) and gt0[0, hi2] in (-1, -2)
    cen = census(A, Bd, gt0, gt1)
    assert cen["min_hinge"] >= MIN_HINGE, cen["min_hinge"]
    for f, low, high in (("triplet01", lo, hi), ("unmatched0", lo, hi), ("triplet10", lo2, hi2), ("unmatched1", lo2, hi2)):
        gaps, win, args = cen["gaps"][f], cen["winners"][f], cen["args"][f]
        tied = gaps == 0
        assert bool(((gaps >= MIN_GAP) | tied).all()), (f, float(gaps[~tied].min()))
        assert int(tied.sum()) >= 1 and bool((win[tied][:, 2] == low).all()) and bool((args[tied] > 0).any()), f
        assert int((win[:, 2] == high).sum()) == 0, f
    return cen


def reference64(case, margin, weights=(W_LOSS, W_METRIC)):
    """Float64 autograd of the restatement (tests/supervision_ref.py) on case = (scores, desc0, desc1, gt0, gt1, ...):
    {'loss', 'metric_loss'} as floats and 'grad_scores', 'grad_desc0', 'grad_desc1' (None without a margin) as float64 arrays,
    for the backward pass of weights[0] * loss + weights[1] * metric_loss."""
    S, A, Bd, gt0, gt1 = case[:5]
    S64, a64, b64 = (t.detach().cpu().double().requires_grad_(True) for t in (S, A, Bd))
    lo = ref.criterion(gt0.cpu(), gt1.cpu(), S64, a64, b64, margin)
    (weights[0] * lo["loss"] + weights[1] * lo["metric_loss"]).backward()
    grad = lambda t: None if t.grad is None else t.grad.numpy()
    return {"loss": lo["loss"].item(), "metric_loss": lo["metric_loss"].item(),
            "grad_scores": grad(S64), "grad_desc0": grad(a64), "grad_desc1": grad(b64)}
