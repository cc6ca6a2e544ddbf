#!/usr/bin/env python3
"""The reference's main training stage -- MegaDepth pairs with '3d_reprojection' supervision (train.py, config/config.yaml,
data/megadepth_dataset.py) -- from frames, on openglue_amd:

    uint8 frames, depth maps, K, R, T --megadepth.megadepth_pairs-->  image0, image1, transformation   (random crops drawn on the CPU)
    --augment weak_color_aug: augment.augment on image0, image1 of the training items (never on the validation item)
    SuperPoint (or --features sift) on both views                  -> LAFs, responses, descriptors
    examples/train_step.py training_step: prepare_features_output -> generate_gt_matches -> SuperGlue.train() -> criterion
    backward -> openglue_amd.optim.Adam (clip + Adam + StepLR), the constants of examples/train_fit.py
    one validation step: centre crops -> SuperGlue.match -> metrics (epipolar precision, pose AUC), as examples/validate.py

The scene is synthetic and seeded: a textured plane at depth Z seen by two cameras with the same orientation, the second one shifted
sideways and with another focal length, so that frame 1 is frame 0's texture at another scale and offset, and K0, K1, R = I, T and the
constant depth maps describe it exactly (a plane under a small sideways baseline leaves the relative pose nearly undetermined, so the
validation's pose AUC says nothing here; the precision of the ground-truth labels, 1, is the line that checks the geometry).  Every
frame of the batch has its own size, as MegaDepth's have; they stand for what a loader hands over after decoding.  From there to the
parameter update every tensor stays on the GPU.

    python examples/train_megadepth.py [--steps 5] [--pairs 2] [--target 320 240] [--features superpoint|sift] [--augment none|weak_color_aug]"""
import argparse
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from examples.pretrain_homography import extract, make_extractor      # noqa: E402
from examples.train_fit import GAMMA, LR, MAX_GRAD_NORM                # noqa: E402
from examples.train_step import MARGIN, NEG_THR, POS_THR, training_step    # noqa: E402
from examples.validate import AUC_THR, EPI_THR, RANSAC_THR             # noqa: E402
from openglue_amd import augment, features, megadepth, metrics, optim, supervision, synthetic as syn    # noqa: E402
from openglue_amd.superglue import SuperGlue                           # noqa: E402

DEPTH = 5.0


def make_scene(B, target, dev, seed=0):
    """-> frames0, frames1, depth0, depth1 (lists of B device tensors of differing sizes), K0, K1, R, T"""
    g = torch.Generator().manual_seed(seed)
    tw, th = target
    r = lambda lo, hi: int(torch.randint(lo, hi, (1,), generator=g))
    frames0, frames1, K0, K1, T = [], [], [], [], []
    for b in range(B):
        W0, H0 = tw + r(tw // 3, tw), th + r(th // 8, th // 2)               # every frame its own size and aspect ratio
        W1, H1 = tw + r(tw // 8, tw // 2), th + r(th // 3, th)
        s = 0.8 + 0.4 * float(torch.rand(1, generator=g))                    # focal length of camera 1 over camera 0
        sw, sh = int(round(W1 / s)), int(round(H1 / s))                      # the part of the texture frame 1 sees
        base = torch.cat([syn.make_image(max(H0, sh) + 40, max(W0, sw) + 40, seed=seed + 3 * b + c) for c in range(3)], dim=1)     # [1, 3, h, w]
        o0, o1 = (r(0, 40), r(0, 40)), (r(0, 40), r(0, 40))
        f0 = base[0, :, o0[1]:o0[1] + H0, o0[0]:o0[0] + W0]
        f1 = F.interpolate(base[:, :, o1[1]:o1[1] + sh, o1[0]:o1[0] + sw], size=(H1, W1), mode="bilinear", align_corners=False, antialias=s < 1)[0]
        sx, sy = W1 / sw, H1 / sh                                            # the scales actually applied (rounded extents)
        f = 1.2 * W0
        t = 0.2 * torch.randn(2, generator=g)
        # p1 + 0.5 = s (p0 + o0 - o1 + 0.5)  and  p1 = K1 (Z K0^-1 p0 + T) / Z
        c0 = (W0 / 2, H0 / 2)
        c1 = [sc * (a - b_ + 0.5) - 0.5 + sc * c - sc * f * float(tt) / DEPTH for sc, a, b_, c, tt in zip((sx, sy), o0, o1, c0, t)]
        frames0.append((f0 * 255).round().to(torch.uint8).permute(1, 2, 0).contiguous().to(dev))
        frames1.append((f1.clamp(0, 1) * 255).round().to(torch.uint8).permute(1, 2, 0).contiguous().to(dev))
        K0.append(torch.tensor([[f, 0, c0[0]], [0, f, c0[1]], [0, 0, 1]]))
        K1.append(torch.tensor([[sx * f, 0, c1[0]], [0, sy * f, c1[1]], [0, 0, 1]]))
        T.append(torch.tensor([float(t[0]), float(t[1]), 0.0]))
    depth = lambda frames: [torch.full(fr.shape[:2], DEPTH, device=dev) for fr in frames]
    R = torch.eye(3).repeat(B, 1, 1)
    return frames0, frames1, depth(frames0), depth(frames1), torch.stack(K0).to(dev), torch.stack(K1).to(dev), R.to(dev), torch.stack(T).to(dev)


def run(steps=5, n_pairs=2, target=(320, 240), feature="superpoint", keypoints=512, stages=3, seed=0, log=print, augmentation="none"):
    """-> ([(matched labels, total loss)] per step, the validation metrics)"""
    dev = torch.device("cuda:0")
    scene = make_scene(n_pairs, target, dev, seed)
    log("frames " + ", ".join(f"{a.shape[1]}x{a.shape[0]} / {b.shape[1]}x{b.shape[0]}" for a, b in zip(scene[0], scene[1])) + f" -> {target[0]}x{target[1]}")
    extractor, dim = make_extractor(feature, keypoints, dev)
    cfg = syn.make_config(descriptor_dim=dim, num_stages=stages, num_heads=4, num_iters=20, side_info_size=1)
    model = SuperGlue(cfg)
    model.load_state_dict(syn.make_state_dict(cfg, seed=0))
    model = model.to(dev).train()
    opt = optim.Adam(model.parameters(), lr=LR, max_grad_norm=MAX_GRAD_NORM, scheduler_gamma=GAMMA)
    gen = torch.Generator().manual_seed(seed)                  # the crop starts are drawn on the CPU
    transform = augment.get_augmentation_transform({"name": augmentation})
    aug_gen = torch.Generator(device=dev).manual_seed(seed)    # the augmentation on the device
    history = []
    for s in range(steps):
        item = augment.augment(megadepth.megadepth_pairs(*scene, target, random_crop=True, generator=gen), transform, aug_gen)
        with torch.no_grad():
            batch = extract(extractor, item)
        opt.zero_grad(set_to_none=False)
        out = training_step(model, batch, MARGIN, with_labels=True)
        if out is None:                                   # an image without keypoints: the reference skips the batch too
            log(f"step {s:2d}  no keypoints, skipped")
            continue
        total, lo, y_true = out
        total.backward()
        opt.step()
        matched = int((y_true["gt_matches0"] >= 0).sum())
        history.append((matched, float(total.detach())))
        log(f"step {s:2d}  keypoints {batch['lafs0'].shape[1]} / {batch['lafs1'].shape[1]} per image  matched labels {matched}  "
            f"loss {history[-1][1]:.4f}  nll {float(lo['loss'].detach()):.4f}  metric {float(lo['metric_loss'].detach()):.4f}")
    # validation: centre crops, the model's matches and the ground-truth labels through the metrics
    model.eval()
    item = megadepth.megadepth_pairs(*scene, target)
    with torch.no_grad():
        batch = extract(extractor, item)
        f0 = features.prepare_features_output(batch["lafs0"], batch["scores0"], batch["descriptors0"], "none")
        f1 = features.prepare_features_output(batch["lafs1"], batch["scores1"], batch["descriptors1"], "none")
        data, y = supervision.generate_gt_matches(batch, f0, f1, POS_THR, NEG_THR, apply_thresholds=True)
        pred = model.match(data, 0.2)
    result = {}
    for name, m0 in (("model", pred["matches0"]), ("ground truth", y["gt_matches0"])):
        acc, auc = metrics.AccuracyUsingEpipolarDist(EPI_THR), metrics.CameraPoseAUC(AUC_THR, RANSAC_THR)
        for metric in (acc, auc):
            metric.update_batch(data["keypoints0"], data["keypoints1"], m0, item["transformation"])
        result[name] = {k: float(v) for k, v in {**acc.compute(), **auc.compute()}.items()}
        log(f"validation {name:>12}: matched {int((m0 >= 0).sum())}  " + "  ".join(f"{k} {v:.4f}" for k, v in result[name].items()))
    return history, result


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--pairs", type=int, default=2)
    ap.add_argument("--target", type=int, nargs=2, default=(320, 240), metavar=("W", "H"))
    ap.add_argument("--features", default="superpoint", choices=("superpoint", "sift"))
    ap.add_argument("--keypoints", type=int, default=512)
    ap.add_argument("--augment", default="none", choices=("none", "weak_color_aug"))
    a = ap.parse_args()
    run(a.steps, a.pairs, tuple(a.target), a.features, a.keypoints, augmentation=a.augment)
