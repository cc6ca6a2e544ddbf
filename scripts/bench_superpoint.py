"""SuperPointNetBn (2048 keypoints) on HIP vs the ATen / MIOpen fp32 formulation of the same network and selection, same GPU,
alternating, one process.  Prints ms / image and images / s per (B, H, W), and checks that both keep the same keypoints under the
exemption rule of tests/test_gpu_superpoint.py (keypoints within 4e-5 of a decision flip, counted against the float64 heatmap
of the ATen run's inputs, may differ).

    python scripts/bench_superpoint.py [--iters 20] [--shapes 1x480x640,16x480x640,1x720x960,16x720x960]
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import superpoint_ref as R  # noqa: E402

from openglue_amd import synthetic as syn  # noqa: E402
from openglue_amd.superpoint import SuperPointNetBn  # noqa: E402

THR, K = 0.005, 2048


def aten_forward(sd, img):
    """The reference's formulation in fp32 ATen: convolutions (MIOpen), softmax, NMS by max over shifted views, top-k, sampling."""
    heat, desc = R.dense(sd, img, dtype=torch.float32)
    keep = (heat > R.max_neighbours(heat, 9)) & (heat > THR)
    keep[:, :4], keep[:, -4:], keep[:, :, :4], keep[:, :, -4:] = False, False, False, False
    out = []
    for b in range(img.shape[0]):
        idx = torch.nonzero(keep[b].flatten()).flatten()
        sc = heat[b].flatten()[idx]
        if K < len(idx):
            sc, o = torch.topk(sc, K)
            idx = idx[o]
        out.append((idx, sc))
    n = min(len(i) for i, _ in out)
    res = []
    for b, (idx, sc) in enumerate(out):
        if any(len(i) != n for i, _ in out):
            sc, o = torch.topk(sc, n)
            idx = idx[o]
        Wh = heat.shape[2]
        xy = torch.stack([idx % Wh, idx // Wh], 1).float()
        p = (xy - 4 + 0.5) / torch.tensor([Wh - 4.5, heat.shape[1] - 4.5], device=img.device) * 2 - 1
        d = torch.nn.functional.grid_sample(desc[b].permute(2, 0, 1)[None], p.view(1, 1, -1, 2), align_corners=False)
        res.append((idx, sc, torch.nn.functional.normalize(d.view(256, -1), dim=0).t()))
    return heat, res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--shapes", default="1x480x640,16x480x640,1x720x960,16x720x960")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    sd = syn.make_superpoint_state_dict(True, seed=1)
    net = SuperPointNetBn(max_keypoints=K, keypoint_threshold=THR)
    net.load_state_dict(sd)
    net = net.eval().to(dev)
    sdd = {k: v.to(dev) for k, v in sd.items()}
    for shape in a.shapes.split(","):
        B, H, W = (int(v) for v in shape.split("x"))
        img = torch.cat([syn.make_image(H, W, seed=500 + i) for i in range(min(B, 4))]).repeat((B + 3) // 4, 1, 1, 1)[:B].to(dev)
        lafs, scores, _ = net(img)
        heat_a, res = aten_forward(sdd, img)
        torch.cuda.synchronize()
        # same keypoints under the exemption rule (margins from the float64 heatmap of the first image)
        h64, _ = R.dense({k: v.cpu() for k, v in sd.items()}, img[:1].cpu())
        _, margin = R.pixel_decisions(h64, 9, 4, THR)
        Wh = h64.shape[2]
        g = set((lafs[0, :, 1, 2].long() * Wh + lafs[0, :, 0, 2].long()).tolist())
        t = set(res[0][0].tolist())
        kth = float(scores[0].min()) if scores.shape[1] else 0.0
        diff = {i for i in g ^ t if not (margin.flatten()[i] < 4e-5 or abs(float(h64.flatten()[i]) - kth) < 4e-5)}
        times = {"hip": [], "aten": []}
        for _ in range(a.iters):
            for name, fn in (("hip", lambda: net(img)), ("aten", lambda: aten_forward(sdd, img))):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                times[name].append(time.perf_counter() - t0)
        med = {k: sorted(v)[len(v) // 2] * 1e3 for k, v in times.items()}
        print(json.dumps({"B": B, "H": H, "W": W, "keypoints": int(scores.shape[1]),
                          "hip_ms_per_image": round(med["hip"] / B, 4), "hip_images_per_s": round(B / med["hip"] * 1e3, 1),
                          "aten_ms_per_image": round(med["aten"] / B, 4), "aten_images_per_s": round(B / med["aten"] * 1e3, 1),
                          "speedup": round(med["aten"] / med["hip"], 2), "unexplained_keypoint_differences_image0": len(diff)}),
              flush=True)
        assert not diff, sorted(diff)[:10]


if __name__ == "__main__":
    main()
