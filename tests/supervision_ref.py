"""Float64 restatement of the reference's training supervision (models/gt_matches_generation.py with utils/misc.py:21-103, and
utils/losses.py), for the tests of openglue_amd.supervision.  Plain torch on any device.

Ground-truth matches: the same statements as csrc/supervision.hip, as float64 torch ops in the same order -- the 3x3 inverses
by the adjugate, each matrix row as (A_r0 x0 + A_r1 x1) + A_r2 x2, squared distances as dx * dx + dy * dy, the first index on
ties -- so that the HIP labels equal these on every row.  `nn_gaps` also returns the gap between the best and the second-best
candidate, which bounds where the reference's own fp32 `torch.cdist` may pick another neighbour.

Criterion: the oracle's restatement (oracle/superglue_oracle.py: nll_criterion, metric_criterion) in whatever dtype it is given.
"""
from __future__ import annotations

import torch

from oracle.superglue_oracle import metric_criterion, nll_criterion

EPS_W = 1e-8


def inv3(a: torch.Tensor) -> torch.Tensor:
    """[B, 3, 3] -> [B, 3, 3] float64 inverse by the adjugate (reproject_kernel's inv3)."""
    a = a.to(torch.float64)
    e = [[a[:, r, c] for c in range(3)] for r in range(3)]
    c00 = e[1][1] * e[2][2] - e[1][2] * e[2][1]
    c01 = e[1][2] * e[2][0] - e[1][0] * e[2][2]
    c02 = e[1][0] * e[2][1] - e[1][1] * e[2][0]
    det = e[0][0] * c00 + e[0][1] * c01 + e[0][2] * c02
    o = [c00 / det, (e[0][2] * e[2][1] - e[0][1] * e[2][2]) / det, (e[0][1] * e[1][2] - e[0][2] * e[1][1]) / det,
         c01 / det, (e[0][0] * e[2][2] - e[0][2] * e[2][0]) / det, (e[0][2] * e[1][0] - e[0][0] * e[1][2]) / det,
         c02 / det, (e[0][1] * e[2][0] - e[0][0] * e[2][1]) / det, (e[0][0] * e[1][1] - e[0][1] * e[1][0]) / det]
    return torch.stack(o, dim=1).reshape(-1, 3, 3)


def mv3(A: torch.Tensor, x0, x1, x2):
    """rows of A [B, 3, 3] (float64) applied to the vectors (x0, x1, x2), each [B, n]: a list of three [B, n]."""
    return [A[:, r, 0, None] * x0 + A[:, r, 1, None] * x1 + A[:, r, 2, None] * x2 for r in range(3)]


def depth_at(depth: torch.Tensor, kpts: torch.Tensor) -> torch.Tensor:
    """utils/misc.py:76-85: per-keypoint depth, or the map read at the truncated coordinates (torch indexing: IndexError out of range)."""
    if depth.dim() == 2:
        return depth
    idx = kpts.type(torch.int64)
    B = kpts.shape[0]
    return depth[torch.arange(B, device=kpts.device).unsqueeze(-1), idx[..., 1], idx[..., 0]]


def reproject(kpts: torch.Tensor, tr: dict, inverse: bool):
    """keypoints [B, n, 2] (fp32) mapped into the other image, float64 [B, n, 2], and the valid mask [B, n]."""
    ttype = tr["type"][0]
    x, y = kpts[..., 0].to(torch.float64), kpts[..., 1].to(torch.float64)
    one = torch.ones_like(x)
    if ttype == "perspective":
        H = inv3(tr["H"]) if inverse else tr["H"].to(torch.float64)
        q = mv3(H, x, y, one)
        valid = torch.ones_like(x, dtype=torch.bool)
    elif ttype == "3d_reprojection":
        Ka, Kb = (tr["K1"], tr["K0"]) if inverse else (tr["K0"], tr["K1"])
        R = tr["R"].to(torch.float64)
        T = tr["T"].to(torch.float64)
        if inverse:
            R = R.transpose(1, 2)
            T = torch.stack([-(R[:, r, 0] * T[:, 0] + R[:, r, 1] * T[:, 1] + R[:, r, 2] * T[:, 2]) for r in range(3)], dim=1)
        d = depth_at(tr["depth1"] if inverse else tr["depth0"], kpts)
        valid = ~torch.isclose(d, d.new_tensor(0.0))
        d = d.to(torch.float64)
        p = mv3(inv3(Ka), x, y, one)
        p = [v * d for v in p]
        r3 = mv3(R, *p)
        r3 = [r3[k] + T[:, k, None] for k in range(3)]
        q = mv3(Kb.to(torch.float64), *r3)
    else:
        raise ValueError(f"Unknown transformation type {ttype}.")
    w = q[2] + EPS_W
    return torch.stack([q[0] / w, q[1] / w], dim=-1), valid


def nn_gaps(q: torch.Tensor, t: torch.Tensor, chunk: int = 1024):
    """nearest neighbour of every query q [B, nq, 2] (float64) among t [B, nt, 2] (fp32): (d2 [B, nq], index [B, nq] -- first on
    ties, gap [B, nq] = second-best minus best squared distance (inf with one candidate))."""
    t = t.to(torch.float64)
    d2s, idxs, gaps = [], [], []
    for s in range(0, q.shape[1], chunk):
        qc = q[:, s:s + chunk]
        dx = qc[..., 0, None] - t[:, None, :, 0]
        dy = qc[..., 1, None] - t[:, None, :, 1]
        d2 = dx * dx + dy * dy
        mn, ix = d2.min(dim=2)
        if d2.shape[2] > 1:
            two = d2.topk(2, dim=2, largest=False).values
            gap = two[..., 1] - two[..., 0]
        else:
            gap = torch.full_like(mn, float("inf"))
        d2s.append(mn); idxs.append(ix); gaps.append(gap)
    return torch.cat(d2s, 1), torch.cat(idxs, 1), torch.cat(gaps, 1)


def gt_matches(kpts0, kpts1, tr, positive_threshold, negative_threshold=None, apply_thresholds=False, with_details=False):
    """labels (gt_matches0 [B, m], gt_matches1 [B, n]) as og_gt_matches computes them; with_details adds a dict of the
    intermediate nearest-neighbour results (nn0, nn1, d2_0, d2_1, gap0, gap1, q0, q1, valid0, valid1)."""
    if negative_threshold is None:
        negative_threshold = positive_threshold
    q0, v0 = reproject(kpts0, tr, False)
    q1, v1 = reproject(kpts1, tr, True)
    d2_0, nn0, gap0 = nn_gaps(q0, kpts1)
    d2_1, nn1, gap1 = nn_gaps(q1, kpts0)
    m, n = nn0.shape[1], nn1.shape[1]
    mut0 = nn1.gather(1, nn0) == torch.arange(m, device=nn0.device)
    mut1 = nn0.gather(1, nn1) == torch.arange(n, device=nn1.device)
    gt0 = torch.where(mut0, nn0, torch.full_like(nn0, -1))
    gt1 = torch.where(mut1, nn1, torch.full_like(nn1, -1))
    if apply_thresholds:
        dist0, dist1 = d2_0.sqrt(), d2_1.sqrt()
        sym0 = 0.5 * (dist0 + dist1.gather(1, nn0))          # mutual pair (i, nn0[i]): its own two distances
        sym1 = 0.5 * (dist0.gather(1, nn1) + dist1)
        gt0[mut0 & (sym0 > positive_threshold)] = -2
        gt0[mut0 & (sym0 > negative_threshold)] = -1
        gt1[mut1 & (sym1 > positive_threshold)] = -2
        gt1[mut1 & (sym1 > negative_threshold)] = -1
        gt0[~mut0 & (dist0 <= negative_threshold)] = -2
        gt1[~mut1 & (dist1 <= negative_threshold)] = -2
    gt0[~v0] = -2
    gt1[~v1] = -2
    if apply_thresholds:
        gt0[mut0 & ~v1.gather(1, nn0)] = -2
        gt1[mut1 & ~v0.gather(1, nn1)] = -2
    if not with_details:
        return gt0, gt1
    return gt0, gt1, dict(nn0=nn0, nn1=nn1, d2_0=d2_0, d2_1=d2_1, gap0=gap0, gap1=gap1, q0=q0, q1=q1, valid0=v0, valid1=v1)


def near_tie_rows(kpts0, kpts1, det, rel=1e-6, abs_px2=1e-3):
    """rows whose label the reference's fp32 arithmetic may legitimately choose differently: the squared-distance gap between
    the best and second-best candidate is below the rounding bound of fp32 cdist / reprojection, rel * (|q|^2 + max |t|^2) +
    abs_px2 (torch.cdist's matrix-product form: 0.06 px^2 at coordinates near 1000).  A row is exempt if its own choice or its
    neighbour's choice (the mutual check) is such a near tie."""
    def bound(q, t):
        qq = (q * q).sum(-1)
        tt = (t.to(torch.float64) ** 2).sum(-1).amax(dim=1, keepdim=True)
        return rel * (qq + tt) + abs_px2
    near0 = det["gap0"] < bound(det["q0"], kpts1)
    near1 = det["gap1"] < bound(det["q1"], kpts0)
    ex0 = near0 | near1.gather(1, det["nn0"])
    ex1 = near1 | near0.gather(1, det["nn1"])
    return ex0, ex1


def criterion(gt0, gt1, scores, ctx0=None, ctx1=None, margin=None):
    """utils/losses.py criterion restated: {'loss', 'metric_loss'} (metric_loss 0 without a margin)."""
    loss = nll_criterion(scores, gt0, gt1)
    if margin is None:
        return {"loss": loss, "metric_loss": torch.zeros((), dtype=scores.dtype, device=scores.device)}
    return {"loss": loss, "metric_loss": metric_criterion(ctx0, ctx1, gt0, gt1, margin)}
