#!/usr/bin/env python3
"""Time one update_batch of AccuracyUsingEpipolarDist and of CameraPoseAUC (1000 hypotheses) at B = 1 and B = 32 pairs of
1024 keypoints (70 % of them matched, 30 % of the matches outliers), device events around `--iters` calls after a warm-up.
The kernels each call launches are fixed (1 and 5 whatever B); count them in a trace with
    rocprofv3 --kernel-trace --stats -d <dir> -- python scripts/bench_metrics.py --iters 5

    python scripts/bench_metrics.py [--iters 20] [--hypotheses 1000]"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from openglue_amd import metrics          # noqa: E402
from tests.test_gpu_metrics import make_scene   # noqa: E402


def timed(fn, iters):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--hypotheses", type=int, default=1000)
    ap.add_argument("--kpts", type=int, default=1024)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    for B in (1, 32):
        t0 = time.perf_counter()
        k0, k1, m0, tr, _ = make_scene(B, a.kpts, outliers=0.3, noise=0.5, seed=B)
        print(f"B={B}: scene built in {time.perf_counter() - t0:.1f} s", file=sys.stderr, flush=True)
        g = torch.Generator().manual_seed(0)
        m0[torch.rand(B, a.kpts, generator=g) < 0.3] = -1
        k0, k1, m0 = k0.to(dev), k1.to(dev), m0.to(dev)
        tr = {k: v.float().to(dev) for k, v in tr.items()}
        acc = metrics.AccuracyUsingEpipolarDist()
        auc = metrics.CameraPoseAUC([5.0, 10.0, 20.0], 1.0, hypotheses=a.hypotheses)
        t_acc = timed(lambda: acc.update_batch(k0, k1, m0, tr), a.iters)
        t_auc = timed(lambda: auc.update_batch(k0, k1, m0, tr), a.iters)
        print(json.dumps({"pairs": B, "keypoints": a.kpts, "hypotheses": a.hypotheses, "epipolar_ms": round(t_acc, 4),
                          "pose_auc_ms": round(t_auc, 4), "launches_epipolar": 1, "launches_pose": 5,
                          "auc": {k: round(float(v), 4) for k, v in auc.compute().items()}}), flush=True)


if __name__ == "__main__":
    main()
