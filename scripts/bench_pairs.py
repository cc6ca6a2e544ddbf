#!/usr/bin/env python3
"""Time the synthesis of homography training pairs (data/oxford_paris_dataset.py:32-66 for a batch) on one GPU:

    hip:   openglue_amd.pairs.homography_pairs (two launches: both 8 x 8 solves of every pair, then both views)
    aten:  the same item from ATen operators: the two systems by torch.linalg.solve (float64), torch.linalg.inv, a sampling grid,
           grid_sample(bilinear, zeros, align_corners=True) of the float frame, crop, grey, / 255

at the reference's operating point (config/homography_pretraining.yaml: 4 frames of 1232 x 1472 x 3, offset 256) and at one
480 x 640 frame (offset 48).  Both run in one process, alternating, REPEATS repeats; device events around STEPS calls after WARMUP
calls; the corner displacements are given (drawn once), so both do the same work.  Also the launches per call of each
(kernel_trace.launched_kernels), the algorithmic bytes -- every frame byte once, 8 bytes written per output pixel -- as a share of the
8 TB/s HBM peak, and the largest difference between the two results (the ATen one interpolates in float, not at 1/32 pixel).
Needs an MI355X: without a GPU it fails.

    python scripts/bench_pairs.py            # STEPS=200 WARMUP=20 REPEATS=3 (environment)"""
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from openglue_amd import kernel_trace, pairs      # noqa: E402

STEPS = int(os.environ.get("STEPS", 200)); WARMUP = int(os.environ.get("WARMUP", 20)); REPEATS = int(os.environ.get("REPEATS", 3))
HBM_PEAK = 8e12

if not torch.cuda.is_available():
    sys.exit("bench_pairs.py needs an MI355X: no GPU is visible (there is no CPU path to fall back to)")
dev = torch.device("cuda:0")


def solve(src, dst):
    """[B, 4, 2] float32 -> [B, 3, 3] float64: cv2.getPerspectiveTransform's system by torch.linalg.solve"""
    s, d = src.double(), dst.double()
    x, y, u, v = s[..., 0], s[..., 1], d[..., 0], d[..., 1]
    one, zero = torch.ones_like(x), torch.zeros_like(x)
    A = torch.cat([torch.stack([x, y, one, zero, zero, zero, -x * u, -y * u], -1), torch.stack([zero, zero, zero, x, y, one, -x * v, -y * v], -1)], 1)
    h = torch.linalg.solve(A, torch.cat([u, v], 1))
    return torch.cat([h, torch.ones_like(h[:, :1])], 1).view(-1, 3, 3)


def aten_pairs(frames, offset, warp_offset):
    B, H, W, C = frames.shape
    o = offset
    c = torch.tensor([[o, o], [o, H - o - 1], [W - o - 1, o], [W - o - 1, H - o - 1]], dtype=torch.float32, device=frames.device).expand(B, 4, 2)
    H_warp = solve(c + warp_offset, c)
    H_true = solve(c - o + warp_offset, c - o).float()
    yy, xx = torch.meshgrid(torch.arange(H, device=frames.device, dtype=torch.float64), torch.arange(W, device=frames.device, dtype=torch.float64), indexing="ij")
    p = torch.stack([xx, yy, torch.ones_like(xx)], -1).view(1, H * W, 3) @ torch.linalg.inv(H_warp).transpose(1, 2)
    grid = torch.stack([p[..., 0] / p[..., 2] / (W - 1) * 2 - 1, p[..., 1] / p[..., 2] / (H - 1) * 2 - 1], -1).view(B, H, W, 2).float()
    x = frames.permute(0, 3, 1, 2).float()
    warped = torch.nn.functional.grid_sample(x, grid, mode="bilinear", padding_mode="zeros", align_corners=True)
    wgt = torch.tensor([0.299, 0.587, 0.114], device=frames.device).view(1, 3, 1, 1)
    grey = lambda t: ((t[:, :, o:H - o, o:W - o] * wgt).sum(1, keepdim=True) / 255.0)
    return {"image0": grey(x), "image1": grey(warped), "transformation": {"type": ["perspective"] * B, "H": H_true}}


def timed(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / n


for B, H, W, offset in ((4, 1232, 1472, 256), (1, 480, 640, 48)):
    g = torch.Generator(device=dev).manual_seed(0)
    frames = torch.randint(0, 256, (B, H // 8, W // 8, 3), device=dev, generator=g, dtype=torch.uint8)
    frames = frames.repeat_interleave(8, 1).repeat_interleave(8, 2).contiguous()        # 8 x 8 blocks: edges to interpolate across
    wo = torch.randint(-offset, offset, (B, 4, 2), device=dev, generator=g).float()
    fns = {"hip": lambda: pairs.homography_pairs(frames, offset, wo), "aten": lambda: aten_pairs(frames, offset, wo)}
    out = {k: f() for k, f in fns.items()}
    launches = {k: kernel_trace.launched_kernels(f) for k, f in fns.items()}
    ms = {k: [] for k in fns}
    for r in range(REPEATS):
        for k, f in fns.items():
            timed(f, WARMUP)
            torch.cuda.synchronize()
            ms[k].append(timed(f, STEPS))
    h, w = H - 2 * offset, W - 2 * offset
    bytes_algo = B * H * W * 3 + 8 * B * h * w
    print(f"homography_pairs, {B} frames of {H} x {W} x 3, offset {offset} -> 2 x [{B}, 1, {h}, {w}]; {STEPS} calls after {WARMUP} warm-up, {REPEATS} repeats, alternating")
    for k in fns:
        med = statistics.median(ms[k])
        print(f"  {k:4s}: {med:.4f} ms per call (repeats {' '.join(f'{v:.4f}' for v in ms[k])}); {len(launches[k])} launches per call; "
              f"{bytes_algo / 1e6:.1f} MB algorithmic = {bytes_algo / (med * 1e-3) / 1e12:.3f} TB/s = {100 * bytes_algo / (med * 1e-3) / HBM_PEAK:.1f} % of the 8 TB/s HBM peak "
              f"(bound {bytes_algo / HBM_PEAK * 1e6:.1f} us)")
    print("  hip launches: " + ", ".join(launches["hip"]))
    spread = max(max(v) - min(v) for v in ms.values())
    print(f"  hip / aten = {statistics.median(ms['hip']) / statistics.median(ms['aten']):.3f}; largest spread between repeats of one code {spread:.4f} ms")
    d1 = (out["hip"]["image1"] - out["aten"]["image1"]).abs()
    print(f"  image0 max |hip - aten| {float((out['hip']['image0'] - out['aten']['image0']).abs().max()):.4f}, image1 max {float(d1.max()):.4f} mean {float(d1.mean()):.5f} "
          f"(grey levels / 255); H max |hip - aten| {float((out['hip']['transformation']['H'] - out['aten']['transformation']['H']).abs().max()):.2e}")
    del frames, out
    torch.cuda.empty_cache()
