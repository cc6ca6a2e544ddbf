"""DoG + AffNet + OriNet + HardNet (openglue_amd/affnet_hardnet.py, 2048 keypoints) per stage and in total, next to the SIFT extractor
(2048 keypoints) on the same images, one process, alternating.  Stage times are host clocks around a stage that ends in a device
synchronise (medians); a total is one forward call, which synchronises once.  Each net is timed on the patches the pipeline feeds it
(already normalised by the extraction); its rate counts 2 * MACs of the convolutions.

    python scripts/bench_patchnets.py [--iters 20] [--shapes 1x480x640,2x480x640] [--out profiles/patchnets_bench.jsonl]
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
from openglue_amd.affnet_hardnet import DoGAffNetHardNet, PatchPyramid  # noqa: E402
from openglue_amd.sift import SIFT  # noqa: E402

K = 2048


def net_flop(kind):
    c = 32 if kind == "hardnet" else 16
    nout = {"hardnet": 128, "affnet": 3, "orinet": 2}[kind]
    convs = [(1, c, 32), (c, c, 32), (c, 2 * c, 16), (2 * c, 2 * c, 16), (2 * c, 4 * c, 8), (4 * c, 4 * c, 8)]
    return 2 * (sum(9 * ci * co * so * so for ci, co, so in convs) + 64 * 4 * c * nout)


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
    ap.add_argument("--shapes", default="1x480x640,2x480x640")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "patchnets_bench.jsonl"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    model = DoGAffNetHardNet(max_keypoints=K)
    model.hardnet.load_state_dict(syn.make_patchnet_state_dict("hardnet", seed=1))
    model.affnet.load_state_dict(syn.make_patchnet_state_dict("affnet", seed=1))
    model.orinet.angle_detector.load_state_dict(syn.make_patchnet_state_dict("orinet", seed=1))
    model = model.to(dev)
    sift = SIFT(max_keypoints=K)
    lines = []
    for shape in a.shapes.split(","):
        B, H, W = (int(v) for v in shape.split("x"))
        img = torch.cat([(syn.make_image(H, W, seed=500 + i) * 255).round() / 255 for i in range(B)]).to(torch.float32).to(dev)
        for _ in range(2):                     # warm-up: code objects, packing, allocator
            model(img)
            sift(img)
        t = {}
        t["detect"], (lafs, _) = timed(lambda: model.detect(img), a.iters)
        n = lafs.shape[1]
        t["pyramid"], pyr = timed(lambda: PatchPyramid(img), a.iters)
        t["extract"], patches = timed(lambda: pyr.extract(lafs, normalize=True), a.iters)
        flat = lafs.reshape(B * n, 2, 3)
        nets = {"affnet": model.affnet, "orinet": model.orinet.angle_detector, "hardnet": model.hardnet}
        rate = {}
        for kind, net in nets.items():
            scratch = flat.clone()
            t[kind], _ = timed(lambda: net.run(patches, None if kind == "hardnet" else scratch, normalize=False), a.iters)
            rate[kind] = round(net_flop(kind) * B * n / t[kind] / 1e9, 2)
        t["describe"], _ = timed(lambda: model.describe(img, lafs), a.iters)
        total, sift_total = [], []
        for _ in range(a.iters):               # alternating
            total.append(timed(lambda: model(img), 1)[0])
            sift_total.append(timed(lambda: sift(img), 1)[0])
        total, sift_total = sorted(total)[len(total) // 2], sorted(sift_total)[len(sift_total) // 2]
        line = json.dumps({"B": B, "H": H, "W": W, "keypoints": n, "stage_ms": {k: round(v, 4) for k, v in t.items()},
                           "net_TFLOP_per_s": rate, "total_ms": round(total, 4), "ms_per_image": round(total / B, 4),
                           "sift_total_ms": round(sift_total, 4)})
        print(line, flush=True)
        lines.append(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
