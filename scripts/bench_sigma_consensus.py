#!/usr/bin/env python3
"""Time scoring="sigma" next to the default scoring="inliers" for geometry.fundamental_matrix and geometry.homography in one process:
B = 1 and B = 32 pairs of 2048 keypoints (70 % of them matched, 30 % of the matches outliers, 0.5 px noise), 2048 hypotheses, refine 0
and 2, each model on a scene of its own.  Plain and sigma-consensus run at the same threshold (1 px for F, 2 px for H), and
sigma-consensus also at the generous 8 px it is meant for, where many more (model, match) pairs reach the table.  The calls of a row
alternate; each figure is the mean of `--iters` calls between device events, taken in three repeats after a warm-up, the median and the
spread of the repeats are written.  Every call is four launches; the kernels' own times come from
    rocprofv3 --kernel-trace --stats -d <dir> -- python scripts/bench_sigma_consensus.py --iters 5
One JSON row per (pairs, refine) goes to stdout and, with --out, to that file (profiles/sigma_consensus_bench.jsonl is the committed run).

    python scripts/bench_sigma_consensus.py [--iters 20] [--kpts 2048] [--hypotheses 2048] [--out profiles/sigma_consensus_bench.jsonl]"""
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
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--kpts", type=int, default=2048)
    ap.add_argument("--hypotheses", type=int, default=2048)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_sigma_consensus.py needs a GPU: a time taken anywhere else says nothing")
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
        for refine in (0, 2):
            kw = dict(hypotheses=H, refine=refine)
            fns = {
                "fundamental_plain_ms": lambda: geometry.fundamental_matrix(*fs, threshold=1.0, **kw),
                "fundamental_sigma_ms": lambda: geometry.fundamental_matrix(*fs, threshold=1.0, scoring="sigma", **kw),
                "fundamental_sigma_8px_ms": lambda: geometry.fundamental_matrix(*fs, threshold=8.0, scoring="sigma", **kw),
                "homography_plain_ms": lambda: geometry.homography(*hs, threshold=2.0, **kw),
                "homography_sigma_ms": lambda: geometry.homography(*hs, threshold=2.0, scoring="sigma", **kw),
                "homography_sigma_8px_ms": lambda: geometry.homography(*hs, threshold=8.0, scoring="sigma", **kw),
            }
            for fn in fns.values():           # warm-up: allocator, code objects
                fn()
            torch.cuda.synchronize()
            runs = {k: [] for k in fns}
            for _ in range(a.repeats):
                for k, fn in fns.items():     # alternate: drift hits all six alike
                    runs[k].append(timed(fn, a.iters))
            out = {"pairs": B, "keypoints": a.kpts, "hypotheses": H, "refine": refine, "iters": a.iters, "repeats": a.repeats}
            for k, v in runs.items():
                out[k] = round(statistics.median(v), 4)
                out[k.replace("_ms", "_spread_ms")] = round(max(v) - min(v), 4)
            out["matches"] = int((fs[2] >= 0).sum())
            for k in ("fundamental_plain_ms", "fundamental_sigma_ms", "fundamental_sigma_8px_ms"):
                r = fns[k]()
                out[k.replace("_ms", "_inliers")] = int(r["num_inliers"].sum())
                if "quality" in r:
                    out[k.replace("_ms", "_quality")] = round(float(r["quality"].sum()), 2)
            out["launches_per_call"] = 4
            print(json.dumps(out), flush=True)
            rows.append(out)
    if a.out:
        with open(a.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
