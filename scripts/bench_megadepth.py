#!/usr/bin/env python3
"""Time the MegaDepth training item (data/megadepth_dataset.py:119-192 for a batch) on one GPU:

    hip:   openglue_amd.megadepth.megadepth_pairs (one table copy, two launches: the 2 B grey crops and K, then the 2 B depth crops)
    aten:  the same item from ATen operators, frame by frame as the sizes differ: grey as a weighted channel sum, F.interpolate(bilinear,
           align_corners=False) of the whole image and of the whole depth map, slicing, / 255, the K product, torch.stack

at the reference's operating point (config/config.yaml: batches of 4 pairs, target 960 x 720) with frames of roughly 1600 x 1200 of
differing sizes, and at one pair.  Both run in one process, alternating, REPEATS repeats; device events around STEPS calls after WARMUP
calls; centre crops, so both do the same work.  Also the launches per call of each (kernel_trace.launched_kernels), the algorithmic
bytes -- the source rows the crop window touches once (C bytes per pixel of the frame, 4 of the depth map) plus 8 bytes written per
output pixel -- as a share of the 8 TB/s HBM peak, and the largest difference between the two results (ATen interpolates in float).
Needs an MI355X: without a GPU it fails.

    python scripts/bench_megadepth.py            # STEPS=200 WARMUP=20 REPEATS=3 (environment)"""
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from openglue_amd import kernel_trace, megadepth      # noqa: E402

STEPS = int(os.environ.get("STEPS", 200)); WARMUP = int(os.environ.get("WARMUP", 20)); REPEATS = int(os.environ.get("REPEATS", 3))
HBM_PEAK = 8e12
TARGET = (960, 720)
SIZES = [((1600, 1200), (1600, 1067)), ((1600, 1064), (1200, 1600)), ((1536, 1152), (1600, 1000)), ((1600, 1198), (1421, 1600))]     # (w, h) of image 0 / 1

if not torch.cuda.is_available():
    sys.exit("bench_megadepth.py needs an MI355X: no GPU is visible (there is no CPU path to fall back to)")
dev = torch.device("cuda:0")
GREY = torch.tensor([0.299, 0.587, 0.114], device=dev)


def aten_item(frame, depth, K, plan):
    tw, th = TARGET
    rw, rh, axis, start = plan
    H, W = depth.shape
    g = (frame.float() @ GREY)[None, None]
    image = F.interpolate(g, size=(rh, rw), mode="bilinear", align_corners=False)[0, 0]
    d = F.interpolate(depth[None, None], size=(rh, rw), mode="bilinear", align_corners=False)[0, 0]
    S = torch.tensor([[rw / W, 0, 0], [0, rh / H, 0], [0, 0, 1]], device=dev)
    shift = torch.zeros(3, 3, device=dev)
    shift[axis, 2] = start
    if axis == 0:
        image, d = image[:, start:start + tw], d[:, start:start + tw]
    else:
        image, d = image[start:start + th], d[start:start + th]
    return image / 255.0, d, S @ K - shift


def aten_pairs(frames0, frames1, depth0, depth1, K0, K1, R, T, plans):
    B = len(frames0)
    sides = []
    for k, (frames, depths, Ks) in enumerate(((frames0, depth0, K0), (frames1, depth1, K1))):
        items = [aten_item(f, d, K, plans[k * B + i]) for i, (f, d, K) in enumerate(zip(frames, depths, Ks))]
        sides.append([torch.stack([it[j] for it in items]) for j in range(3)])
    (i0, d0, k0), (i1, d1, k1) = sides
    return {"image0": i0[:, None], "image1": i1[:, None],
            "transformation": {"type": ["3d_reprojection"] * B, "K0": k0, "K1": k1, "R": R, "T": T, "depth0": d0, "depth1": d1}}


def timed(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / n


def touched(size, plan):
    """source pixels whose rows and columns the crop window reads"""
    (w, h), (rw, rh, axis, start) = size, plan
    fx, fy = (TARGET[0] / rw, 1.0) if axis == 0 else (1.0, TARGET[1] / rh)
    return int(w * fx) * int(h * fy)


for B in (4, 1):
    g = torch.Generator(device=dev).manual_seed(0)
    sizes = [s[0] for s in SIZES[:B]] + [s[1] for s in SIZES[:B]]

    def frame(w, h):                                              # 8 x 8 blocks: edges to interpolate across
        f = torch.randint(0, 256, ((h + 7) // 8, (w + 7) // 8, 3), device=dev, generator=g, dtype=torch.uint8)
        return f.repeat_interleave(8, 0).repeat_interleave(8, 1)[:h, :w].contiguous()
    frames = [frame(w, h) for w, h in sizes]
    depths = [1.0 + 20.0 * torch.rand(h, w, device=dev, generator=g) for w, h in sizes]
    K = torch.stack([torch.tensor([[1.2 * w, 0, w / 2], [0, 1.2 * w, h / 2], [0, 0, 1]]) for w, h in sizes]).to(dev)
    R, T = torch.eye(3, device=dev).repeat(B, 1, 1), torch.zeros(B, 3, device=dev)
    plans = [megadepth.crop_plan(s, TARGET) for s in sizes]
    args = (frames[:B], frames[B:], depths[:B], depths[B:], K[:B], K[B:], R, T)
    fns = {"hip": lambda: megadepth.megadepth_pairs(*args, TARGET), "aten": lambda: aten_pairs(*args, plans)}
    out = {k: f() for k, f in fns.items()}
    launches = {k: kernel_trace.launched_kernels(f) for k, f in fns.items()}
    ms = {k: [] for k in fns}
    for r in range(REPEATS):
        for k, f in fns.items():
            timed(f, WARMUP)
            torch.cuda.synchronize()
            ms[k].append(timed(f, STEPS))
    bytes_algo = sum(touched(s, p) * (3 + 4) for s, p in zip(sizes, plans)) + 2 * B * TARGET[0] * TARGET[1] * 8
    print(f"megadepth_pairs, {B} pairs, frames {' '.join(f'{w}x{h}' for w, h in sizes)} -> 2 x [{B}, 1, {TARGET[1]}, {TARGET[0]}] + depth; "
          f"{STEPS} calls after {WARMUP} warm-up, {REPEATS} repeats, alternating")
    for k in fns:
        med = statistics.median(ms[k])
        print(f"  {k:4s}: {med:.4f} ms per call (repeats {' '.join(f'{v:.4f}' for v in ms[k])}); {len(launches[k])} launches per call; "
              f"{bytes_algo / 1e6:.1f} MB algorithmic = {bytes_algo / (med * 1e-3) / 1e12:.3f} TB/s = {100 * bytes_algo / (med * 1e-3) / HBM_PEAK:.1f} % of the 8 TB/s HBM peak "
              f"(bound {bytes_algo / HBM_PEAK * 1e6:.1f} us)")
    print("  hip launches: " + ", ".join(launches["hip"]))
    spread = max(max(v) - min(v) for v in ms.values())
    print(f"  hip / aten = {statistics.median(ms['hip']) / statistics.median(ms['aten']):.3f}; largest spread between repeats of one code {spread:.4f} ms")
    h_, a_ = out["hip"], out["aten"]
    print(f"  image0 max |hip - aten| {float((h_['image0'] - a_['image0']).abs().max()) * 255:.3f} grey levels, "
          f"depth0 max {float((h_['transformation']['depth0'] - a_['transformation']['depth0']).abs().max()):.2e}, "
          f"K0 max {float((h_['transformation']['K0'] - a_['transformation']['K0']).abs().max()):.2e}")
    del frames, depths, out
    torch.cuda.empty_cache()
