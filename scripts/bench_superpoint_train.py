"""Forward + backward of SuperPointNet in train() mode on HIP (csrc/superpoint_train.hip) vs the ATen / MIOpen fp32 formulation of the
same network under torch autograd (tests/superpoint_ref.dense in fp32 on the device, heatmap gather, grid_sample, F.normalize), same
GPU, alternating, one process.  Both differentiate sum(scores * Gs) + sum(descriptors * Gd) at the keypoints of the HIP forward, so the
ATen side does no selection at all (which favours it).  Per (B, H, W): median ms of forward and of backward, peak device memory of one
forward + backward, kernel launches per iteration (torch.profiler), and the worst relative gradient difference between the two.
--check64 also differentiates the float64 formulation on the CPU (B = 1 shapes only; seconds) and reports each side's worst relative
gradient error against it: at this size pool and ReLU decisions that fall differently in fp32 dominate both.

    python scripts/bench_superpoint_train.py [--iters 20] [--shapes 1x480x640,4x480x640] [--keypoints 1024] [--check64]
"""
import argparse
import json
import os
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import superpoint_ref as R  # noqa: E402

from openglue_amd import synthetic as syn  # noqa: E402
from openglue_amd.superpoint import CONV_NAMES, SuperPointNet  # noqa: E402

THR = 0.005


def aten_forward(sd, img, xy, dtype=torch.float32):
    heat, desc = R.dense(sd, img, dtype=dtype)
    B, Hh, Wh = heat.shape
    idx = (xy[..., 1] * Wh + xy[..., 0]).long()
    scores = heat.flatten(1).gather(1, idx)
    p = (xy.to(dtype) - 4 + 0.5) / torch.tensor([Wh - 4.5, Hh - 4.5], device=img.device, dtype=dtype) * 2 - 1
    d = F.grid_sample(desc.permute(0, 3, 1, 2), p[:, None], mode="bilinear", align_corners=False)[:, :, 0]       # [B, 256, n]
    return scores, F.normalize(d, p=2, dim=1).transpose(1, 2)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, time.perf_counter() - t0


def launches(fn):
    """device kernels of one call, or None where the profiler is unavailable"""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        return sum(1 for e in prof.events() if str(e.device_type).endswith("CUDA") and "memcpy" not in e.name.lower() and "memset" not in e.name.lower())
    except Exception:                                # noqa: BLE001 -- a missing profiler must not lose the timings
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--shapes", default="1x480x640,4x480x640")
    ap.add_argument("--keypoints", type=int, default=1024)
    ap.add_argument("--check64", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    sd = syn.make_superpoint_state_dict(False, seed=1)
    net = SuperPointNet(max_keypoints=a.keypoints, keypoint_threshold=THR)
    net.load_state_dict(sd)
    net = net.to(dev).train()
    sdd = {k: v.to(dev).requires_grad_(True) for k, v in sd.items()}
    for shape in a.shapes.split(","):
        B, H, W = (int(v) for v in shape.split("x"))
        img = torch.cat([syn.make_image(H, W, seed=500 + i) for i in range(B)]).to(dev)
        lafs, scores, desc = net(img)
        n = scores.shape[1]
        xy = lafs[..., 2].detach()
        g = torch.Generator(device=dev).manual_seed(0)
        Gs, Gd = torch.randn(B, n, device=dev, generator=g), torch.randn(B, n, 256, device=dev, generator=g)

        def hip_fwd():
            return net(img)

        def aten_fwd():
            return aten_forward(sdd, img, xy)

        def bwd(out):
            s, d = out[-2], out[-1]
            torch.autograd.backward([s, d], [Gs, Gd])

        def clear():
            net.zero_grad(set_to_none=True)
            for v in sdd.values():
                v.grad = None

        # same gradients (fp32 vs fp32: summation order only)
        clear()
        bwd(hip_fwd())
        bwd(aten_fwd())
        worst = 0.0
        for name in CONV_NAMES:
            for k in ("weight", "bias"):
                ga, gh = sdd[f"{name}.{k}"].grad, getattr(getattr(net, name), k).grad
                worst = max(worst, float((ga - gh).abs().max() / ga.abs().max()))
        err64 = {}
        if a.check64 and B == 1:
            sd64 = {k: v.double().requires_grad_(True) for k, v in sd.items()}
            s64, d64 = aten_forward(sd64, img.cpu(), xy.cpu(), torch.float64)
            torch.autograd.backward([s64, d64], [Gs.cpu().double(), Gd.cpu().double()])
            for side in ("hip", "aten"):
                err64[side + "_worst_rel_err_vs_fp64"] = float("%.3g" % max(
                    float(((sdd[f"{n_}.{k}"].grad if side == "aten" else getattr(getattr(net, n_), k).grad).cpu().double() - sd64[f"{n_}.{k}"].grad).abs().max()
                          / sd64[f"{n_}.{k}"].grad.abs().max()) for n_ in CONV_NAMES for k in ("weight", "bias")))
        times = {k: [] for k in ("hip_fwd", "hip_bwd", "aten_fwd", "aten_bwd")}
        for it in range(a.iters + 3):                # three warm-up rounds, both sides alternating
            for side, fwd in (("hip", hip_fwd), ("aten", aten_fwd)):
                clear()
                out, tf = timed(fwd)
                _, tb = timed(lambda: bwd(out))
                if it >= 3:
                    times[side + "_fwd"].append(tf)
                    times[side + "_bwd"].append(tb)
                del out
        peak, count = {}, {}
        for side, fwd in (("hip", hip_fwd), ("aten", aten_fwd)):
            clear()
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            base = torch.cuda.memory_allocated(dev)
            torch.cuda.reset_peak_memory_stats(dev)
            bwd(fwd())
            torch.cuda.synchronize()
            peak[side] = (torch.cuda.max_memory_allocated(dev) - base) / 2 ** 20
            clear()
            count[side] = launches(lambda: bwd(fwd()))
        med = {k: sorted(v)[len(v) // 2] * 1e3 for k, v in times.items()}
        print(json.dumps({"B": B, "H": H, "W": W, "keypoints": n,
                          **{k + "_ms": round(v, 3) for k, v in med.items()},
                          "hip_total_ms": round(med["hip_fwd"] + med["hip_bwd"], 3), "aten_total_ms": round(med["aten_fwd"] + med["aten_bwd"], 3),
                          "speedup": round((med["aten_fwd"] + med["aten_bwd"]) / (med["hip_fwd"] + med["hip_bwd"]), 2),
                          "hip_peak_MiB": round(peak["hip"], 1), "aten_peak_MiB": round(peak["aten"], 1),
                          "hip_kernels": count["hip"], "aten_kernels": count["aten"], "worst_rel_grad_diff": float(f"{worst:.3g}"), **err64}), flush=True)


if __name__ == "__main__":
    main()
