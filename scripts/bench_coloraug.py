#!/usr/bin/env python3
"""Time weak_color_aug (utils/augmentations.py: RandomEqualize, RandomSharpness, RandomSolarize, RandomGaussianNoise on a batch) on one GPU:

    hip:         openglue_amd.augment.color_aug_packed: og_color_aug alone, three launches (histogram, table, apply), the tables packed once
    hip+pack:    openglue_amd.augment.color_aug: the same after packing the drawn parameters into the three tables (a few small ATen launches)
    aten:        the same four functions from ATen operators the way kornia runs them: each operation on the flagged samples (boolean
                 indexing), equalize per plane with torch.histc, cumsum, gather and a host-side `step == 0`, conv2d, where, randn

at 4 x 1 x 720 x 960 (a MegaDepth batch of the reference's size) and 1 x 1 x 480 x 640, (a) with all four flags on every sample and (b)
with a seeded draw at the default probabilities.  All run in one process, alternating, REPEATS repeats; device events around STEPS calls
after WARMUP calls.  Also the launches per call of each (kernel_trace.launched_kernels) and the algorithmic bytes -- every pixel read once
and written once, 8 bytes, plus one more read of the samples that are equalized -- as a share of the 8 TB/s HBM peak.  The ATen result
differs from the kernels' in the noise (another random stream) only; the other three stages are compared.
Needs an MI355X: without a GPU it fails.

    python scripts/bench_coloraug.py            # STEPS=200 WARMUP=20 REPEATS=3 (environment)"""
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from openglue_amd import augment, kernel_trace      # noqa: E402

STEPS = int(os.environ.get("STEPS", 200)); WARMUP = int(os.environ.get("WARMUP", 20)); REPEATS = int(os.environ.get("REPEATS", 3))
HBM_PEAK = 8e12

if not torch.cuda.is_available():
    sys.exit("bench_coloraug.py needs an MI355X: no GPU is visible (there is no CPU path to fall back to)")
dev = torch.device("cuda:0")


def aten_equalize_plane(im):
    im = im * 255.0
    histo = torch.histc(im, bins=256, min=0, max=255)
    nonzero_histo = torch.reshape(histo[histo != 0], [-1])
    step = (torch.sum(nonzero_histo) - nonzero_histo[-1]) // 255
    if step == 0:
        return im / 255.0
    lut = torch.div(torch.cumsum(histo, 0) + torch.div(step, 2, rounding_mode="trunc"), step, rounding_mode="trunc")
    lut = torch.clamp(torch.cat([torch.zeros(1, device=lut.device, dtype=lut.dtype), lut[:-1]]), 0, 255)
    return torch.gather(lut, 0, im.flatten().long()).reshape_as(im) / 255.0


def aten_sharpness(x, factor):
    C = x.shape[1]
    kernel = torch.tensor([[1, 1, 1], [1, 5, 1], [1, 1, 1]], dtype=x.dtype, device=x.device).view(1, 1, 3, 3).repeat(C, 1, 1, 1) / 13
    blur = torch.clamp(torch.nn.functional.conv2d(x, kernel, groups=C), 0.0, 1.0)
    mask = torch.nn.functional.pad(torch.ones_like(blur), [1, 1, 1, 1])
    result = torch.where(mask == 1, torch.nn.functional.pad(blur, [1, 1, 1, 1]), x)
    return result + (x - result) * factor.view(-1, 1, 1, 1)             # 0 < factor < 1 here: no special cases, no clamp


def aten_color_aug(x, p, noise=True):
    x = x.clone()
    on = p["equalize"]
    if on.any():
        x[on] = torch.stack([torch.stack([aten_equalize_plane(pl) for pl in img]) for img in x[on]])
    on = p["sharpness"]
    if on.any():
        x[on] = aten_sharpness(x[on], p["factor"][on])
    on = p["solarize"]
    if on.any():
        t = torch.clamp(x[on] + p["addition"][on].view(-1, 1, 1, 1), 0.0, 1.0)
        x[on] = torch.where(t < p["threshold"][on].view(-1, 1, 1, 1), t, 1.0 - t)
    on = p["noise"]
    if noise and on.any():
        x[on] = x[on] + (p["noise_mean"][on].view(-1, 1, 1, 1) + p["noise_std"][on].view(-1, 1, 1, 1) * torch.randn_like(x[on]))
    return x


def timed(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / n


for B, C, H, W in ((4, 1, 720, 960), (1, 1, 480, 640)):
    g = torch.Generator(device=dev).manual_seed(0)
    coarse = torch.rand(B, C, H // 8, W // 8, device=dev, generator=g)
    image = torch.nn.functional.interpolate(coarse, size=(H, W), mode="bilinear", align_corners=False)       # smooth, as a photograph is
    image = ((image + 0.1 * torch.rand(B, C, H, W, device=dev, generator=g)) / 1.1 * 255).round().div(255).contiguous()
    drawn = augment.sample_weak_color_aug(B, dev, torch.Generator(device=dev).manual_seed(1))
    every = {k: (torch.ones_like(v) if v.dtype == torch.bool else v) for k, v in drawn.items()}
    for case, p in (("all four flags on every sample", every), ("a seeded draw at the default probabilities", drawn)):
        tables = augment.pack_params(p)
        fns = {"hip": lambda: augment.color_aug_packed(image, *tables), "hip+pack": lambda: augment.color_aug(image, p), "aten": lambda: aten_color_aug(image, p)}
        launches = {k: kernel_trace.launched_kernels(f) for k, f in fns.items()}
        ms = {k: [] for k in fns}
        for r in range(REPEATS):
            for k, f in fns.items():
                timed(f, WARMUP)
                torch.cuda.synchronize()
                ms[k].append(timed(f, STEPS))
        n_eq = int(p["equalize"].sum())
        bytes_algo = 4 * C * H * W * (2 * B + n_eq)
        flags = [int(v) for v in tables[0].tolist()]
        print(f"weak_color_aug, {B} x {C} x {H} x {W}, {case} (flags {flags}); {STEPS} calls after {WARMUP} warm-up, {REPEATS} repeats, alternating")
        for k in fns:
            med = statistics.median(ms[k])
            print(f"  {k:8s}: {med:.4f} ms per call (repeats {' '.join(f'{v:.4f}' for v in ms[k])}); {len(launches[k])} launches per call; "
                  f"{bytes_algo / 1e6:.1f} MB algorithmic = {bytes_algo / (med * 1e-3) / 1e12:.3f} TB/s = {100 * bytes_algo / (med * 1e-3) / HBM_PEAK:.1f} % of the 8 TB/s HBM peak "
                  f"(bound {bytes_algo / HBM_PEAK * 1e6:.1f} us)")
        print("  hip launches: " + ", ".join(launches["hip"]))
        spread = max(max(v) - min(v) for v in ms.values())
        print(f"  hip / aten = {statistics.median(ms['hip']) / statistics.median(ms['aten']):.3f}; hip+pack / aten = "
              f"{statistics.median(ms['hip+pack']) / statistics.median(ms['aten']):.3f}; largest spread between repeats of one code {spread:.4f} ms")
        quiet = {**p, "noise": torch.zeros_like(p["noise"])}
        d = (augment.color_aug(image, quiet) - aten_color_aug(image, quiet, noise=False)).abs()
        print(f"  without the noise: max |hip - aten| {float(d.max()):.3e}, pixels that differ {int((d > 0).sum())} of {d.numel()}")
    del image
    torch.cuda.empty_cache()
