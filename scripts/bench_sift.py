"""The SIFT extractor (openglue_amd/sift.py, 2048 keypoints) per stage and in total, next to SuperPointNetBn (2048 keypoints) at the
same sizes, one process, alternating.  Stage times are host clocks around a stage that ends in a device synchronise (medians); the
total is one forward call, which synchronises once.  The pyramid's achieved bandwidth is its algorithmic bytes -- the image read
once, every Gaussian level read once (as the source of the next) and written once, every DoG layer written once -- over its time.

    python scripts/bench_sift.py [--iters 20] [--shapes 1x480x640,2x480x640,1x720x960,2x720x960]
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from openglue_amd import synthetic as syn  # noqa: E402
from openglue_amd.sift import SIFT, geometry  # noqa: E402
from openglue_amd.superpoint import SuperPointNetBn  # noqa: E402

K = 2048


def pyramid_bytes(B, H, W):
    geom = geometry(H, W)
    px = sum(h * w for h, w in geom.octaves)
    # image in, upsampled image out and in; per octave 6 levels written, 5 read as a source, 5 DoG layers written, 1 decimation read
    return 4 * B * (H * W + 2 * 4 * H * W + px * (6 + 5 + 5) + sum(h * w for h, w in geom.octaves[1:]))


def timed(fn, iters):
    ts = []
    for _ in range(iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return sorted(ts)[len(ts) // 2] * 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--shapes", default="1x480x640,2x480x640,1x720x960,2x720x960")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    sp = SuperPointNetBn(max_keypoints=K, keypoint_threshold=0.005)
    sp.load_state_dict(syn.make_superpoint_state_dict(True, seed=1))
    sp = sp.eval().to(dev)
    net = SIFT(max_keypoints=K)
    for shape in a.shapes.split(","):
        B, H, W = (int(v) for v in shape.split("x"))
        img = torch.cat([(syn.make_image(H, W, seed=500 + i) * 255).round() / 255 for i in range(B)]).to(torch.float32).to(dev)
        geom = geometry(H, W)
        for _ in range(2):                     # warm-up: code objects, allocator
            net(img)
            sp(img)
        ws, counts = net.workspace(B, H, W, dev), net.new_counts(B, dev)
        t = {}
        t["pyramid"], (gauss, dog) = timed(lambda: net.pyramid(img, ws), a.iters)
        t["detect"], (det_i, det_f) = timed(lambda: net.detect(dog, H, W, counts, ws), a.iters)
        t["orient"], (ori_i, ori_f) = timed(lambda: net.orient(gauss, H, W, det_i, det_f, counts, ws), a.iters)
        t["describe"], desc = timed(lambda: net.describe(gauss, H, W, ori_i, ori_f, counts), a.iters)
        t["select"], sel = timed(lambda: net.select(H, W, ori_i, ori_f, counts, ws), a.iters)
        n = net.check_counts(counts.cpu(), B, geom)
        t["gather"], _ = timed(lambda: net.gather(H, W, n, sel, ori_f, desc), a.iters)
        total, sp_total = [], []
        for _ in range(a.iters):               # alternating
            total.append(timed(lambda: net(img), 1)[0])
            sp_total.append(timed(lambda: sp(img), 1)[0])
        total, sp_total = sorted(total)[len(total) // 2], sorted(sp_total)[len(sp_total) // 2]
        c = counts.cpu().tolist()
        print(json.dumps({"B": B, "H": H, "W": W, "detected": c[:B], "oriented": c[B:2 * B], "keypoints": n,
                          "stage_ms": {k: round(v, 4) for k, v in t.items()}, "sift_total_ms": round(total, 4),
                          "sift_ms_per_image": round(total / B, 4), "superpoint_total_ms": round(sp_total, 4),
                          "pyramid_algorithmic_MB": round(pyramid_bytes(B, H, W) / 1e6, 2),
                          "pyramid_GB_per_s": round(pyramid_bytes(B, H, W) / t["pyramid"] / 1e6, 1)}), flush=True)


if __name__ == "__main__":
    main()
