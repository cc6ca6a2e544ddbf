#!/usr/bin/env python3
"""The reference's training step end to end on openglue_amd (models/matching_module.py:70-105 training_step with cached features):

    LAFs, responses, descriptors --features.prepare_features_output-->  keypoints, side info
    + known transformation       --supervision.generate_gt_matches-->  gt_matches0 / gt_matches1
    SuperGlue(config).train()(data)                                  -> scores, context_descriptors0/1
    supervision.criterion(y_true, y_pred, margin)                    -> loss, metric_loss
    nll_weight * loss + metric_weight * metric_loss  -> backward -> Adam

Every step between the input tensors and the parameter gradients runs on HIP kernels.  The pairs are synthetic: image 1 holds a
jittered copy of 60 % of image 0's keypoints mapped through the transformation -- a homography ('perspective') or poses,
intrinsics and a depth map ('3d_reprojection') -- plus fresh points, with descriptors that agree on the shared points.

    python examples/train_step.py [--steps 20] [--pairs 2] [--kpts 512] [--transform perspective|3d_reprojection]"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from openglue_amd import features, supervision, synthetic as syn       # noqa: E402
from openglue_amd.superglue import SuperGlue                           # noqa: E402

W, H = 640, 480
# config/config.yaml: gt_positive_threshold, gt_negative_threshold, margin, nll_weight, metric_weight
POS_THR, NEG_THR, MARGIN, NLL_WEIGHT, METRIC_WEIGHT = 3.0, 5.0, 0.2, 1.0, 1.0


def _lafs(k, g):
    """LAFs [B, N, 2, 3] centred at k with a random isotropic scale"""
    B, N, _ = k.shape
    s = 2.0 + 6.0 * torch.rand(B, N, generator=g)
    lafs = torch.zeros(B, N, 2, 3)
    lafs[..., 0, 0], lafs[..., 1, 1], lafs[..., 2] = s, s, k
    return lafs


def make_transformation(kind, B, g):
    if kind == "perspective":
        Hm = torch.eye(3).repeat(B, 1, 1)
        Hm[:, :2, :2] += 0.05 * torch.randn(B, 2, 2, generator=g)
        Hm[:, :2, 2] = 10.0 * torch.randn(B, 2, generator=g)
        Hm[:, 2, :2] = 5e-5 * torch.randn(B, 2, generator=g)
        return {"type": ["perspective"] * B, "H": Hm}
    K = torch.tensor([[500.0, 0.0, W / 2], [0.0, 500.0, H / 2], [0.0, 0.0, 1.0]]).repeat(B, 1, 1)
    a = 0.03 * torch.randn(B, generator=g)
    R = torch.eye(3).repeat(B, 1, 1)
    R[:, 0, 0], R[:, 0, 2], R[:, 2, 0], R[:, 2, 2] = a.cos(), a.sin(), -a.sin(), a.cos()
    T = 0.1 * torch.randn(B, 3, generator=g)
    depth0 = 4.0 + torch.rand(B, H, W, generator=g)
    depth0[:, : H // 8] = 0.0                    # a band without depth: those keypoints are ignored
    return {"type": ["3d_reprojection"] * B, "K0": K, "K1": K.clone(), "R": R, "T": T, "depth0": depth0,
            "depth1": 4.0 + torch.rand(B, H, W, generator=g)}


def _map(k, tr):
    """image-0 keypoints into image 1 (utils/misc.py:21-103, float32)"""
    kh = torch.cat([k, torch.ones_like(k[..., :1])], -1)
    if tr["type"][0] == "perspective":
        p = kh @ tr["H"].transpose(1, 2)
    else:
        idx = k.long()
        d = tr["depth0"][torch.arange(k.shape[0])[:, None], idx[..., 1], idx[..., 0]]
        p = (kh @ torch.linalg.inv(tr["K0"]).transpose(1, 2)) * d[..., None]
        p = (p @ tr["R"].transpose(1, 2) + tr["T"][:, None]) @ tr["K1"].transpose(1, 2)
    return p[..., :2] / (p[..., 2:] + 1e-8)


def make_pairs(B, N, D, kind, dev, seed=0):
    g = torch.Generator().manual_seed(seed)
    tr = make_transformation(kind, B, g)
    k0 = torch.rand(B, N, 2, generator=g) * torch.tensor([W - 1.0, H - 1.0])
    k1 = torch.rand(B, N, 2, generator=g) * torch.tensor([W - 1.0, H - 1.0])
    d0 = torch.nn.functional.normalize(torch.randn(B, N, D, generator=g), dim=-1)
    d1 = torch.nn.functional.normalize(torch.randn(B, N, D, generator=g), dim=-1)
    mapped = _map(k0, tr)
    for b in range(B):
        src = torch.randperm(N, generator=g)[: int(0.6 * N)]
        dst = torch.randperm(N, generator=g)[: src.numel()]
        inside = ((mapped[b, src] >= 0) & (mapped[b, src] < torch.tensor([W - 1.0, H - 1.0]))).all(-1)
        src, dst = src[inside], dst[inside]
        k1[b, dst] = mapped[b, src] + 0.7 * torch.randn(src.numel(), 2, generator=g)
        d1[b, dst] = torch.nn.functional.normalize(d0[b, src] + 0.1 * torch.randn(src.numel(), D, generator=g), dim=-1)
    k1 = k1.clamp(min=0.0).minimum(torch.tensor([W - 1.0, H - 1.0]))
    to = lambda t: t.to(dev)
    cached = {"lafs0": to(_lafs(k0, g)), "lafs1": to(_lafs(k1, g)), "scores0": to(torch.rand(B, N, generator=g)),
              "scores1": to(torch.rand(B, N, generator=g)), "descriptors0": to(d0), "descriptors1": to(d1),
              "transformation": {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in tr.items()},
              "image0_size": [W, H], "image1_size": [W, H]}
    return cached


def training_step(model, batch, margin=MARGIN, with_labels=False):
    """matching_module.py:70-105 with use_cached_features: the weighted loss and its two parts (with_labels: and the ground-truth
    labels), or None without keypoints"""
    f0 = features.prepare_features_output(batch["lafs0"], batch["scores0"], batch["descriptors0"], "none")
    f1 = features.prepare_features_output(batch["lafs1"], batch["scores1"], batch["descriptors1"], "none")
    data, y_true = supervision.generate_gt_matches(batch, f0, f1, POS_THR, NEG_THR)
    if data is None:
        return None
    y_pred = model(data)
    lo = supervision.criterion(y_true, y_pred, margin=margin)
    total = NLL_WEIGHT * lo["loss"] + METRIC_WEIGHT * lo["metric_loss"]
    return (total, lo, y_true) if with_labels else (total, lo)


def run(steps=20, pairs=2, kpts=512, dim=128, stages=3, lr=1e-3, transform="perspective", margin=MARGIN, log=print):
    """`steps` Adam steps on one synthetic batch; returns (total losses, {parameter name: its gradient after the first step})"""
    dev = torch.device("cuda:0")
    cfg = syn.make_config(descriptor_dim=dim, num_stages=stages, num_heads=4, num_iters=20, side_info_size=1)
    model = SuperGlue(cfg)
    model.load_state_dict(syn.make_state_dict(cfg, seed=0))
    model = model.to(dev).train()
    opt = torch.optim.Adam(model.parameters(), lr=lr)
    batch = make_pairs(pairs, kpts, dim, transform, dev)
    losses, first_grads = [], None
    t0 = time.perf_counter()
    for s in range(steps):
        opt.zero_grad(set_to_none=True)
        total, lo = training_step(model, batch, margin)
        total.backward()
        if first_grads is None:
            first_grads = {k: (None if p.grad is None else p.grad.detach().clone()) for k, p in model.named_parameters()}
        opt.step()
        losses.append(float(total.item()))
        if s % 5 == 0 or s + 1 == steps:
            log(f"step {s:3d}  total {losses[-1]:.4f}  nll {lo['loss'].item():.4f}  metric {lo['metric_loss'].item():.4f}")
    torch.cuda.synchronize(dev)
    log(f"{steps} steps of {pairs} pairs x {kpts} keypoints ({transform}): {(time.perf_counter() - t0) / steps * 1e3:.1f} ms per step")
    return losses, first_grads


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--pairs", type=int, default=2)
    ap.add_argument("--kpts", type=int, default=512)
    ap.add_argument("--transform", default="perspective", choices=("perspective", "3d_reprojection"))
    a = ap.parse_args()
    run(a.steps, a.pairs, a.kpts, transform=a.transform)
