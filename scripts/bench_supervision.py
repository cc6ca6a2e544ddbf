#!/usr/bin/env python3
"""Time the training step's supervision -- ground-truth labels + criterion forward + backward -- on the HIP path
(openglue_amd.supervision) against the reference's ATen formulation (models/gt_matches_generation.py, utils/misc.py,
utils/losses.py, restated below with the same torch ops), at 4 x 1024 and 2 x 2048 keypoints, D = 128 and 256, with and
without a margin.  Prints one line per case and path: milliseconds per step and the peak torch.cuda.max_memory_allocated
increase over the inputs.

    python scripts/bench_supervision.py [--steps 20] [--warmup 5]"""
import argparse
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from openglue_amd import supervision     # noqa: E402


# ---------------------------------------------------------------- the reference's formulation (ATen ops, as in the reference)
def aten_gt_matches(kpts0, kpts1, H, pos, neg):
    def persp(k, Hm):
        B, n, _ = k.shape
        kh = torch.cat([k, torch.ones(B, n, 1, device=k.device)], 2)
        t = torch.matmul(kh, Hm.transpose(1, 2).contiguous())
        return t[..., :2] / (t[..., 2].unsqueeze(-1) + 1e-8), torch.ones(B, n, dtype=torch.bool, device=k.device)
    t0, mask0 = persp(kpts0, H)
    t1, mask1 = persp(kpts1, torch.linalg.inv(H))
    e01 = torch.cdist(t0, kpts1, p=2)
    e10 = torch.cdist(t1, kpts0, p=2)
    min0, nn0 = e01.min(2)
    min1, nn1 = e10.min(2)
    gt0, gt1 = nn0.clone(), nn1.clone()
    cc0 = torch.arange(kpts0.shape[1], device=gt0.device).unsqueeze(0) == gt1.gather(1, gt0)
    gt0[~cc0] = -1
    cc1 = torch.arange(kpts1.shape[1], device=gt0.device).unsqueeze(0) == gt0.gather(1, gt1)
    gt1[~cc1] = -1
    sym = 0.5 * (min0[cc0] + min1[cc1])
    gt0[cc0][sym > pos] = -2        # (writes into copies, as in the reference)
    gt0[cc0][sym > neg] = -1
    gt1[cc1][sym > pos] = -2
    gt1[cc1][sym > neg] = -1
    gt0[~cc0][min0[~cc0] <= neg] = -2
    gt1[~cc1][min1[~cc1] <= neg] = -2
    gt0[~mask0] = -2
    gt1[~mask1] = -2
    gt0[cc0][~mask1.gather(1, nn0)[cc0]] = -2
    gt1[cc1][~mask0.gather(1, nn1)[cc1]] = -2
    return {"gt_matches0": gt0, "gt_matches1": gt1}


def aten_criterion(y_true, y_pred, margin):
    gt0, gt1 = y_true["gt_matches0"], y_true["gt_matches1"]
    g0, g1, scores = y_pred["context_descriptors0"], y_pred["context_descriptors1"], y_pred["scores"]
    dist = None
    if margin is not None:
        a = F.normalize(g0.transpose(2, 1).contiguous(), dim=-1)
        b = F.normalize(g1.transpose(2, 1).contiguous(), dim=-1)
        dist = 0.25 * torch.cdist(a, b).pow(2)

    def weights(bi):
        _, inv, counts = torch.unique_consecutive(bi, return_inverse=True, return_counts=True)
        return (1 / counts)[inv]
    zero = torch.tensor(0, device=scores.device)
    bi, i0 = torch.where(gt0 >= 0)
    i1 = gt0[bi, i0]
    w = weights(bi)
    matched = (-scores[bi, i0, i1] * w).sum()
    trip = zero
    if margin is not None:
        dap = dist[bi, i0, i1]
        dd = dist.detach().clone()
        dd[bi, i0, i1] = np.inf
        c01, c10 = torch.argmin(dd, dim=1), torch.argmin(dd, dim=2)
        an0, an1 = dist[bi, i0, c10[bi, i0]], dist[bi, c01[bi, i1], i1]
        trip = (torch.maximum(dap - an0 + margin, zero) * w).sum() + (torch.maximum(dap - an1 + margin, zero) * w).sum()
    bi, i0 = torch.where(gt0 == -1)
    w = weights(bi)
    un0 = (-scores[bi, i0, -1] * w).sum()
    m0 = zero if margin is None else (torch.maximum(-dist[bi, i0, torch.argmin(dist, dim=2)[bi, i0]] + margin, zero) * w).sum()
    bi, i1 = torch.where(gt1 == -1)
    w = weights(bi)
    un1 = (-scores[bi, -1, i1] * w).sum()
    m1 = zero if margin is None else (torch.maximum(-dist[bi, torch.argmin(dist, dim=1)[bi, i1], i1] + margin, zero) * w).sum()
    B = scores.size(0)
    return {"loss": (matched + 0.5 * (un0 + un1)) / B, "metric_loss": (trip + m0 + m1) / B}


# ---------------------------------------------------------------- the measurement
def case_inputs(B, N, D, dev, seed=0):
    g = torch.Generator(device=dev).manual_seed(seed)
    k0 = torch.rand(B, N, 2, device=dev, generator=g) * torch.tensor([1280.0, 960.0], device=dev)
    H = torch.eye(3, device=dev).repeat(B, 1, 1)
    H[:, :2, 2] = 5.0
    k1 = k0[:, torch.randperm(N, device=dev, generator=g)] + 5.0 + torch.randn(B, N, 2, device=dev, generator=g)
    S = torch.log_softmax(torch.randn(B, N + 1, N + 1, device=dev, generator=g).reshape(B, -1), -1).reshape(B, N + 1, N + 1)
    return k0, k1, H, S.requires_grad_(True), torch.randn(B, D, N, device=dev, generator=g).requires_grad_(True), \
        torch.randn(B, D, N, device=dev, generator=g).requires_grad_(True)


def step(path, k0, k1, H, S, a, b, margin):
    if path == "hip":
        f = lambda k: {"keypoints": k, "local_descriptors": None, "side_info": None}
        _, y = supervision.generate_gt_matches({"transformation": {"type": ["perspective"] * k0.shape[0], "H": H}}, f(k0), f(k1), 3.0, 5.0)
        lo = supervision.criterion(y, {"scores": S, "context_descriptors0": a, "context_descriptors1": b}, margin=margin)
    else:
        y = aten_gt_matches(k0, k1, H, 3.0, 5.0)
        lo = aten_criterion(y, {"scores": S, "context_descriptors0": a, "context_descriptors1": b}, margin)
    total = lo["loss"] + lo["metric_loss"]
    total.backward()
    S.grad = a.grad = b.grad = None
    return lo, y


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    for B, N in ((4, 1024), (2, 2048)):
        for D in (128, 256):
            for margin in (None, 0.2):
                inp = case_inputs(B, N, D, dev)
                res = {}
                for path in ("hip", "aten"):
                    for _ in range(args.warmup):
                        lo, y = step(path, *inp, margin)
                    torch.cuda.synchronize()
                    torch.cuda.reset_peak_memory_stats()
                    base = torch.cuda.memory_allocated()
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(args.steps):
                        lo, y = step(path, *inp, margin)
                    e1.record()
                    torch.cuda.synchronize()
                    ms = e0.elapsed_time(e1) / args.steps
                    peak = (torch.cuda.max_memory_allocated() - base) / 2**20
                    res[path] = (lo["loss"].item(), lo["metric_loss"].item(), y["gt_matches0"].cpu())
                    print(f"B={B} N={N} D={D} margin={margin}: {path:4s} {ms:8.3f} ms/step  peak +{peak:8.2f} MiB", flush=True)
                agree = float((res["hip"][2] == res["aten"][2]).float().mean())
                print(f"B={B} N={N} D={D} margin={margin}: loss hip {res['hip'][0]:.6f} aten {res['aten'][0]:.6f}; metric hip "
                      f"{res['hip'][1]:.6f} aten {res['aten'][1]:.6f}; gt_matches0 agree on {agree * 100:.2f} % of rows", flush=True)


if __name__ == "__main__":
    main()
