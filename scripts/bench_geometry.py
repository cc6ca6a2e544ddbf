#!/usr/bin/env python3
"""Time geometry.fundamental_matrix (refine 0 and 2) next to metrics.relative_pose on the same matches with the same number of
hypotheses: B = 1 and B = 32 pairs of 2048 keypoints (70 % of them matched, 30 % of the matches outliers, 0.5 px noise), at 1000
and 2048 hypotheses.  The three alternate in one process; each figure is the mean of `--iters` calls between device events, taken
in three repeats after a warm-up, the median and the spread of the repeats are printed.  Launches per call are fixed (4 and 5
whatever B); count them in a trace with
    rocprofv3 --kernel-trace --stats -d <dir> -- python scripts/bench_geometry.py --iters 5

    python scripts/bench_geometry.py [--iters 20] [--kpts 2048]"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from openglue_amd import geometry, metrics      # noqa: E402
from tests.geometry_ref import make_scene       # noqa: E402


def timed(fn, iters):
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
    ap.add_argument("--kpts", type=int, default=2048)
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    for B in (1, 32):
        t0 = time.perf_counter()
        k0, k1, m0, tr, _ = make_scene(B, a.kpts, outliers=0.3, noise=0.5, seed=B)
        print(f"B={B}: scene built in {time.perf_counter() - t0:.1f} s", file=sys.stderr, flush=True)
        g = torch.Generator().manual_seed(0)
        m0[torch.rand(B, a.kpts, generator=g) < 0.3] = -1
        k0, k1, m0 = k0.to(dev), k1.to(dev), m0.to(dev)
        trd = {k: tr[k].float().to(dev) for k in ("K0", "K1", "R", "T")}
        for H in (1000, 2048):
            fns = {
                "fundamental_refine0_ms": lambda: geometry.fundamental_matrix(k0, k1, m0, hypotheses=H, refine=0),
                "fundamental_refine2_ms": lambda: geometry.fundamental_matrix(k0, k1, m0, hypotheses=H, refine=2),
                "relative_pose_ms": lambda: metrics.relative_pose(k0, k1, m0, trd, 1.0, hypotheses=H),
            }
            for fn in fns.values():           # warm-up: allocator, code objects
                fn()
            torch.cuda.synchronize()
            runs = {k: [] for k in fns}
            for _ in range(a.repeats):
                for k, fn in fns.items():     # alternate: drift hits all three alike
                    runs[k].append(timed(fn, a.iters))
            r0 = geometry.fundamental_matrix(k0, k1, m0, hypotheses=H, refine=0)
            r2 = geometry.fundamental_matrix(k0, k1, m0, hypotheses=H, refine=2)
            out = {"pairs": B, "keypoints": a.kpts, "hypotheses": H, "iters": a.iters, "repeats": a.repeats}
            for k, v in runs.items():
                out[k] = round(statistics.median(v), 4)
                out[k.replace("_ms", "_spread_ms")] = round(max(v) - min(v), 4)
            out["inliers_refine0"] = int(r0["num_inliers"].sum())
            out["inliers_refine2"] = int(r2["num_inliers"].sum())
            out["launches_fundamental"], out["launches_pose"] = 4, 5
            print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
