"""Forward + backward of SuperPointNetBn in train() mode on HIP (csrc/superpoint_bn_train.hip) against (a) the same assembly under ATen /
MIOpen fp32 autograd on the same GPU (tests/superpoint_bn_ref.dense_train: F.conv2d, F.batch_norm(training=True), max_pool2d, ...) and
(b) SuperPointNet's step (no BatchNorm, csrc/superpoint_train.hip), all three alternating in one process.  Every side differentiates
sum(scores * Gs) + sum(descriptors * Gd) at the keypoints of the HIP BatchNorm forward; the ATen side does no selection.  Per (B, H, W):
median ms of forward + backward, peak device memory of one step, and for the passes train-mode BatchNorm adds (the statistics finish,
the d beta / d gamma reduction and its finish) their device time from torch.profiler, algorithmic bytes and achieved GB/s.

    python scripts/bench_superpoint_bn_train.py [--iters 20] [--shapes 1x480x640,4x480x640] [--keypoints 1024]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import superpoint_bn_ref as RB  # noqa: E402
from bench_superpoint_train import THR, timed  # noqa: E402

import torch.nn.functional as F  # noqa: E402

from openglue_amd import synthetic as syn  # noqa: E402
from openglue_amd.kernel_trace import short_name  # noqa: E402
from openglue_amd.superpoint import SuperPointNet, SuperPointNetBn  # noqa: E402

ADDED = ("sp_bn_stats_finish_kernel", "sp_bn_reduce_kernel", "sp_bn_reduce_finish_kernel")


def aten_forward(sd, img, xy):
    heat, desc, _ = RB.dense_train(sd, img, dtype=torch.float32)
    B, Hh, Wh = heat.shape
    scores = heat.flatten(1).gather(1, (xy[..., 1] * Wh + xy[..., 0]).long())
    p = (xy - 4 + 0.5) / torch.tensor([Wh - 4.5, Hh - 4.5], device=img.device) * 2 - 1
    d = F.grid_sample(desc.permute(0, 3, 1, 2), p[:, None], mode="bilinear", align_corners=False)[:, :, 0]
    return scores, F.normalize(d, p=2, dim=1).transpose(1, 2)


def added_bytes(B, H, W):
    """algorithmic bytes of the added passes of one step: the reduction reads the layer's raw output once and the incoming gradient once
    (a quarter of the pixels behind a pool); the finishes read the per-tile partials"""
    layers = [(H, W, 64, False), (H, W, 64, True), (H // 2, W // 2, 64, False), (H // 2, W // 2, 64, True), (H // 4, W // 4, 128, False),
              (H // 4, W // 4, 128, True), (H // 8, W // 8, 128, False), (H // 8, W // 8, 128, False), (H // 8, W // 8, 512, False)]
    red = stats = fin = 0
    for i, (h, w, c, pooled) in enumerate(layers):
        n = B * h * w
        red += n * c * 4 + (B * (h // 2) * (w // 2) if pooled else n) * c * 4
        flat = (n + 127) // 128
        tiles = flat if i == 0 else B * ((h + 7) // 8) * ((w + 15) // 16)
        stats += c * tiles * 12
        fin += c * flat * 8
    return {"sp_bn_stats_finish_kernel": stats, "sp_bn_reduce_kernel": red, "sp_bn_reduce_finish_kernel": fin}


def kernel_times(fn):
    """device microseconds of one call: per added kernel (template arguments merged), and every kernel by name (the ten largest and the
    sum are printed: where the step's time goes)"""
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    out, every = {k: 0.0 for k in ADDED}, {}
    for e in prof.events():
        if not str(e.device_type).endswith("CUDA"):
            continue
        name = short_name(e.name)
        t, c = every.get(name, (0.0, 0))
        every[name] = (t + float(getattr(e, "device_time_total", None) or getattr(e, "cuda_time_total", 0.0)), c + 1)
        for k in ADDED:
            if k + "<" in e.name or k + "(" in e.name or e.name.endswith(k):
                out[k] += float(getattr(e, "device_time_total", None) or getattr(e, "cuda_time_total", 0.0))
    return out, every


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--shapes", default="1x480x640,4x480x640")
    ap.add_argument("--keypoints", type=int, default=1024)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    sd = syn.make_superpoint_state_dict(True, seed=1)
    bn = SuperPointNetBn(max_keypoints=a.keypoints, keypoint_threshold=THR)
    bn.load_state_dict(sd)
    bn = bn.to(dev).train()
    plain = SuperPointNet(max_keypoints=a.keypoints, keypoint_threshold=THR)
    plain.load_state_dict(syn.make_superpoint_state_dict(False, seed=1))
    plain = plain.to(dev).train()
    sdd = {k: (v.to(dev).requires_grad_(True) if v.is_floating_point() and "running" not in k else v.to(dev)) for k, v in sd.items()}
    for shape in a.shapes.split(","):
        B, H, W = (int(v) for v in shape.split("x"))
        img = torch.cat([syn.make_image(H, W, seed=500 + i) for i in range(B)]).to(dev)
        lafs, scores, _ = bn(img)
        n, xy = scores.shape[1], lafs[..., 2].detach()
        n_plain = plain(img)[1].shape[1]
        g = torch.Generator(device=dev).manual_seed(0)
        G = {m: (torch.randn(B, m, device=dev, generator=g), torch.randn(B, m, 256, device=dev, generator=g)) for m in {n, n_plain}}

        def step(fwd):
            out = fwd()
            torch.autograd.backward([out[-2], out[-1]], list(G[out[-2].shape[1]]))

        sides = {"hip_bn": lambda: bn(img), "aten_bn": lambda: aten_forward(sdd, img, xy), "hip_plain": lambda: plain(img)}

        def clear():
            bn.zero_grad(set_to_none=True)
            plain.zero_grad(set_to_none=True)
            for v in sdd.values():
                v.grad = None

        times = {k: [] for k in sides}
        for it in range(a.iters + 3):                # three warm-up rounds, the sides alternating
            for side, fwd in sides.items():
                clear()
                _, t = timed(lambda: step(fwd))
                if it >= 3:
                    times[side].append(t)
        peak = {}
        for side, fwd in sides.items():
            clear()
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            base = torch.cuda.memory_allocated(dev)
            torch.cuda.reset_peak_memory_stats(dev)
            step(fwd)
            torch.cuda.synchronize()
            peak[side] = (torch.cuda.max_memory_allocated(dev) - base) / 2 ** 20
        clear()
        (us, every), nbytes = kernel_times(lambda: step(sides["hip_bn"])), added_bytes(B, H, W)
        top = sorted(every.items(), key=lambda kv: -kv[1][0])[:10]
        med = {k: sorted(v)[len(v) // 2] * 1e3 for k, v in times.items()}
        print(json.dumps({"B": B, "H": H, "W": W, "keypoints": n, "keypoints_plain": n_plain,
                          **{k + "_ms": round(v, 3) for k, v in med.items()}, **{k + "_peak_MiB": round(v, 1) for k, v in peak.items()},
                          "added": {k: {"us": round(us[k], 1), "MB": round(nbytes[k] / 1e6, 2),
                                        "GBps": round(nbytes[k] / 1e3 / us[k], 1) if us[k] else None} for k in ADDED},
                          "hip_bn_device_us": round(sum(t for t, _ in every.values()), 1), "hip_bn_launches": sum(c for _, c in every.values()),
                          "hip_bn_top_kernels_us": {k: [round(t, 1), c] for k, (t, c) in top}}), flush=True)


if __name__ == "__main__":
    main()
