#!/usr/bin/env python3
"""Time geometry.homography (refine 0 and 2) next to geometry.fundamental_matrix (refine 0 and 2) in one process, each on a scene of
its own model with the same shape: B = 1 and B = 32 pairs of 2048 keypoints (70 % of them matched, 30 % of the matches outliers,
0.5 px noise), 2048 hypotheses.  The four alternate; each figure is the mean of `--iters` calls between device events, taken in
three repeats after a warm-up, the median and the spread of the repeats are written.  Launches per call are fixed (4 and 4 whatever
B); count them in a trace with
    rocprofv3 --kernel-trace --stats -d <dir> -- python scripts/bench_homography.py --iters 5
One JSON row per batch size goes to stdout and, with --out, to that file (profiles/homography_bench.jsonl is the committed run).

    python scripts/bench_homography.py [--iters 200] [--kpts 2048] [--hypotheses 2048] [--out profiles/homography_bench.jsonl]"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from openglue_amd import geometry               # noqa: E402
from tests import geometry_ref, homography_ref  # noqa: E402


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
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--kpts", type=int, default=2048)
    ap.add_argument("--hypotheses", type=int, default=2048)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_homography.py needs a GPU: a time taken anywhere else says nothing")
    dev = torch.device("cuda:0")
    H = a.hypotheses
    rows = []
    for B in (1, 32):
        t0 = time.perf_counter()
        g = torch.Generator().manual_seed(0)
        holes = torch.rand(B, a.kpts, generator=g) < 0.3
        scenes = {}
        for name, make in (("homography", homography_ref.make_scene), ("fundamental", geometry_ref.make_scene)):
            k0, k1, m0 = make(B, a.kpts, outliers=0.3, noise=0.5, seed=B)[:3]
            m0[holes] = -1
            scenes[name] = (k0.to(dev), k1.to(dev), m0.to(dev))
        print(f"B={B}: scenes built in {time.perf_counter() - t0:.1f} s", file=sys.stderr, flush=True)
        hs, fs = scenes["homography"], scenes["fundamental"]
        fns = {
            "homography_refine0_ms": lambda: geometry.homography(*hs, threshold=2.0, hypotheses=H, refine=0),
            "homography_refine2_ms": lambda: geometry.homography(*hs, threshold=2.0, hypotheses=H, refine=2),
            "fundamental_refine0_ms": lambda: geometry.fundamental_matrix(*fs, hypotheses=H, refine=0),
            "fundamental_refine2_ms": lambda: geometry.fundamental_matrix(*fs, hypotheses=H, refine=2),
        }
        for fn in fns.values():           # warm-up: allocator, code objects
            fn()
        torch.cuda.synchronize()
        runs = {k: [] for k in fns}
        for _ in range(a.repeats):
            for k, fn in fns.items():     # alternate: drift hits all four alike
                runs[k].append(timed(fn, a.iters))
        out = {"pairs": B, "keypoints": a.kpts, "hypotheses": H, "iters": a.iters, "repeats": a.repeats}
        for k, v in runs.items():
            out[k] = round(statistics.median(v), 4)
            out[k.replace("_ms", "_spread_ms")] = round(max(v) - min(v), 4)
        out["matches"] = int((hs[2] >= 0).sum())
        out["inliers_homography_refine0"] = int(fns["homography_refine0_ms"]()["num_inliers"].sum())
        out["inliers_homography_refine2"] = int(fns["homography_refine2_ms"]()["num_inliers"].sum())
        out["launches_homography"], out["launches_fundamental"] = 4, 4
        print(json.dumps(out), flush=True)
        rows.append(out)
    if a.out:
        with open(a.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
