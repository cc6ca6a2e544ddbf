#!/usr/bin/env python3
"""Supervision fixtures FROM THE REFERENCE on CPU (build container only: needs /root/reference).

    python tests/golden/make_golden_supervision.py       # writes tests/golden/supervision.npz

gt_<case>_*: the reference's own generate_gt_matches (models/gt_matches_generation.py, with utils/misc.py's reprojection) on
seeded keypoints and transformations:
  persp    'perspective', M != N, B = 2
  depthkp  '3d_reprojection' with per-keypoint depth [B, N], some depths exactly 0
  depthmap '3d_reprojection' with depth maps [B, H, W] that have holes (0), and keypoints whose truncated coordinates are
           negative (torch indexing wraps them around)
  quirk    identity homography, three points shifted by 8 px, thresholds 3 / 5: the mutual pairs beyond both thresholds
           still come out matched (the reference's threshold writes land on copies)
crit_d<D>_*: inputs; crit_d<D>_{none,margin}_*: the reference's own criterion (utils/losses.py) with margin None and 0.2 at D = 128 and 256, labels with -2 and a
pair without any matched keypoint; L = loss + metric_loss differentiated by autograd -> grad_scores, grad_desc0, grad_desc1.
The two modules import only torch, numpy and utils.misc, so they are imported unchanged."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, "/root/reference")

from models.gt_matches_generation import generate_gt_matches     # noqa: E402
from utils.losses import criterion                               # noqa: E402

POS, NEG = 3.0, 5.0


def homography(g, B):
    H = torch.eye(3).repeat(B, 1, 1)
    H[:, :2, :2] += 0.05 * torch.randn(B, 2, 2, generator=g)
    H[:, :2, 2] = 20.0 * torch.randn(B, 2, generator=g)
    H[:, 2, :2] = 1e-4 * torch.randn(B, 2, generator=g)
    return H


def rotation(g, B, scale=0.05):
    w = scale * torch.randn(B, 3, generator=g)
    Wx = torch.zeros(B, 3, 3)
    Wx[:, 0, 1], Wx[:, 0, 2], Wx[:, 1, 2] = -w[:, 2], w[:, 1], -w[:, 0]
    Wx = Wx - Wx.transpose(1, 2)
    return torch.linalg.matrix_exp(Wx)


def intrinsics(B, f, cx, cy):
    K = torch.zeros(B, 3, 3)
    K[:, 0, 0], K[:, 1, 1], K[:, 0, 2], K[:, 1, 2], K[:, 2, 2] = f, f * 1.01, cx, cy, 1.0
    return K


def features(k):
    B, N, _ = k.shape
    return {"keypoints": k, "local_descriptors": torch.zeros(B, N, 4), "side_info": torch.zeros(B, N, 1)}


def perturbed_copies(k, frac, noise, g, extra, lo, hi):
    """keypoints of the other image: a noisy copy of some of k plus uniform extras (so some rows have a close partner)"""
    B, N, _ = k.shape
    take = int(frac * N)
    c = k[:, torch.randperm(N, generator=g)[:take]] + noise * torch.randn(B, take, 2, generator=g)
    e = lo + (hi - lo) * torch.rand(B, extra, 2, generator=g)
    out = torch.cat([c, e], 1)
    return out[:, torch.randperm(out.shape[1], generator=g)].contiguous()


def gt_cases():
    g = torch.Generator().manual_seed(2024)
    cases = {}
    # perspective, M != N
    B, M = 2, 150
    k0 = torch.rand(B, M, 2, generator=g) * torch.tensor([640.0, 480.0])
    H = homography(g, B)
    k0h = torch.cat([k0, torch.ones(B, M, 1)], 2) @ H.transpose(1, 2)
    k1 = perturbed_copies(k0h[..., :2] / k0h[..., 2:], 0.7, 1.5, g, 65, 0.0, 640.0)
    cases["persp"] = dict(k0=k0, k1=k1, tr={"type": ["perspective"] * B, "H": H})
    # 3d_reprojection, depth per keypoint with zeros
    B, M, N = 2, 120, 100
    K0, K1 = intrinsics(B, 500.0, 320.0, 240.0), intrinsics(B, 520.0, 300.0, 250.0)
    R, T = rotation(g, B), 0.3 * torch.randn(B, 3, generator=g)
    k0 = torch.rand(B, M, 2, generator=g) * torch.tensor([640.0, 480.0])
    k1 = torch.rand(B, N, 2, generator=g) * torch.tensor([640.0, 480.0])
    d0, d1 = 2.0 + 8.0 * torch.rand(B, M, generator=g), 2.0 + 8.0 * torch.rand(B, N, generator=g)
    d0[:, ::9] = 0.0
    d1[:, 3::11] = 0.0
    cases["depthkp"] = dict(k0=k0, k1=k1, tr={"type": ["3d_reprojection"] * B, "K0": K0, "K1": K1, "R": R, "T": T, "depth0": d0, "depth1": d1})
    # 3d_reprojection, depth maps with holes; coordinates in [-12, W) x [-12, H): negative truncated indices wrap
    B, M, N, Hd, Wd = 2, 90, 110, 60, 80
    K0, K1 = intrinsics(B, 70.0, 40.0, 30.0), intrinsics(B, 72.0, 41.0, 29.0)
    R, T = rotation(g, B, 0.02), 0.05 * torch.randn(B, 3, generator=g)
    k0 = torch.rand(B, M, 2, generator=g) * torch.tensor([Wd + 12.0, Hd + 12.0]) - 12.0
    k1 = torch.rand(B, N, 2, generator=g) * torch.tensor([Wd + 12.0, Hd + 12.0]) - 12.0
    dm0 = 3.0 + torch.rand(B, Hd, Wd, generator=g)
    dm1 = 3.0 + torch.rand(B, Hd, Wd, generator=g)
    dm0[:, 10:25, 20:45] = 0.0
    dm1[:, 30:50, 5:30] = 0.0
    dm0[:, -3:, :] = 0.0          # a hole that only the wrapped (negative) rows reach
    cases["depthmap"] = dict(k0=k0, k1=k1, tr={"type": ["3d_reprojection"] * B, "K0": K0, "K1": K1, "R": R, "T": T, "depth0": dm0, "depth1": dm1})
    # the quirk: identity homography, three points shifted by 8 px
    k0 = torch.rand(1, 20, 2, generator=g) * 400.0
    k1 = k0.clone()
    k1[0, :3] += torch.tensor([8.0, 0.0])
    cases["quirk"] = dict(k0=k0, k1=k1, tr={"type": ["perspective"], "H": torch.eye(3)[None]})
    return cases


def crit_labels(B, m, n, g):
    gt0 = torch.full((B, m), -1, dtype=torch.long)
    gt1 = torch.full((B, n), -1, dtype=torch.long)
    k = min(m, n) // 2
    i = torch.randperm(m, generator=g)[:k]
    j = torch.randperm(n, generator=g)[:k]
    gt0[0, i], gt1[0, j] = j, i
    gt0[0, torch.randperm(m, generator=g)[:5]] = -2
    gt1[0, (gt1[0] == -1).nonzero()[:4, 0]] = -2
    gt0[1, torch.randperm(m, generator=g)[:7]] = -2      # pair 1: no matched keypoint at all
    gt1[1, torch.randperm(n, generator=g)[:3]] = -2
    return gt0, gt1


def main():
    out = {}
    for name, c in gt_cases().items():
        data, y = generate_gt_matches({"transformation": c["tr"]}, features(c["k0"]), features(c["k1"]), POS, NEG)
        out[f"gt_{name}_k0"], out[f"gt_{name}_k1"] = c["k0"].numpy(), c["k1"].numpy()
        out[f"gt_{name}_type"] = np.array(c["tr"]["type"][0])
        for key, v in c["tr"].items():
            if key != "type":
                out[f"gt_{name}_{key}"] = v.numpy()
        out[f"gt_{name}_gt0"], out[f"gt_{name}_gt1"] = y["gt_matches0"].numpy(), y["gt_matches1"].numpy()
        g0 = y["gt_matches0"]
        print(name, "matched", int((g0 >= 0).sum()), "unmatched", int((g0 == -1).sum()), "ignored", int((g0 == -2).sum()))
    out["gt_thresholds"] = np.array([POS, NEG])
    g = torch.Generator().manual_seed(7)
    B, m, n = 2, 70, 90
    for D in (128, 256):
        gt0, gt1 = crit_labels(B, m, n, g)
        S = torch.log_softmax(torch.randn(B, m + 1, n + 1, generator=g).reshape(B, -1), -1).reshape(B, m + 1, n + 1)
        A = torch.randn(B, D, m, generator=g)
        Bd = torch.randn(B, D, n, generator=g)
        inp = f"crit_d{D}"
        out[f"{inp}_scores"], out[f"{inp}_desc0"], out[f"{inp}_desc1"] = S.numpy(), A.numpy(), Bd.numpy()
        out[f"{inp}_gt0"], out[f"{inp}_gt1"] = gt0.numpy(), gt1.numpy()
        for margin in (None, 0.2):
            name = f"crit_d{D}_{'none' if margin is None else 'margin'}"
            s_ = S.clone().requires_grad_(True)
            a_, b_ = A.clone().requires_grad_(True), Bd.clone().requires_grad_(True)
            lo = criterion({"gt_matches0": gt0, "gt_matches1": gt1}, {"scores": s_, "context_descriptors0": a_, "context_descriptors1": b_},
                           margin=margin)
            (lo["loss"] + lo["metric_loss"]).backward()
            out[f"{name}_loss"] = np.float32(lo["loss"].item())
            out[f"{name}_metric_loss"] = np.float32(lo["metric_loss"].item())
            out[f"{name}_grad_scores"] = s_.grad.numpy().copy()
            out[f"{name}_margin"] = np.float32(np.nan if margin is None else margin)
            if margin is not None:
                out[f"{name}_grad_desc0"], out[f"{name}_grad_desc1"] = a_.grad.numpy().copy(), b_.grad.numpy().copy()
            print(name, "loss", lo["loss"].item(), "metric", lo["metric_loss"].item())
    np.savez_compressed(os.path.join(HERE, "supervision.npz"), **out)


if __name__ == "__main__":
    main()
