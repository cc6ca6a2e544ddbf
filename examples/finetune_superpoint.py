#!/usr/bin/env python3
"""The reference's training step with `finetune: True` in the features config (models/matching_module.py:29-31,77): the extractor stays
in train(), its parameters keep requires_grad, and the matcher's loss is back-propagated through descriptors and responses into it.

    uint8 frames --pairs.homography_pairs-->  image0, image1, H
    --augment weak_color_aug: augment.augment on image0, image1    (what keeps a fine-tuned detector from fitting the training frames)
    SuperPointNet.train() on both views                           -> LAFs, responses (grad_fn), descriptors (grad_fn)
    examples/train_step.py training_step: prepare_features_output -> generate_gt_matches -> SuperGlue.train() -> criterion
    backward (through SuperGlue, side_info / descriptors, csrc/superpoint_train.hip)
    one openglue_amd.optim.Adam step over the matcher's AND the extractor's parameters

Weights are seeded (no checkpoint is needed); the frames are synthetic, as in examples/pretrain_homography.py.  By default every step
draws the SAME pair, so that the printed loss is one curve; --fresh draws a new pair per step, as a data loader would.

--bn fine-tunes SuperPointNetBn instead (the reference's superpoint_coco / superpoint_kitti configurations): every BatchNorm2d runs on
batch statistics and moves its running buffers (csrc/superpoint_bn_train.hip), and its weight and bias are optimised with the rest.

    python examples/finetune_superpoint.py [--steps 6] [--pairs 2] [--size 240 320] [--offset 24] [--keypoints 256] [--fresh] [--bn]
                                          [--augment none|weak_color_aug]"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from examples.pretrain_homography import extract, make_frames          # noqa: E402
from examples.train_fit import GAMMA, MAX_GRAD_NORM                    # noqa: E402
from examples.train_step import MARGIN, training_step                  # noqa: E402
from openglue_amd import augment, optim, pairs, synthetic as syn       # noqa: E402
from openglue_amd.superglue import SuperGlue                           # noqa: E402
from openglue_amd.superpoint import SuperPointNet, SuperPointNetBn     # noqa: E402


def run(steps=6, n_pairs=2, size=(240, 320), offset=24, keypoints=256, stages=3, lr=1e-4, fresh=False, seed=0, log=print, bn=False, augmentation="none"):
    """-> [(matched labels, total loss, |grad| of conv1a.weight)] per step"""
    dev = torch.device("cuda:0")
    H, W = size
    frames = make_frames(n_pairs, H, W, dev, seed)
    extractor = (SuperPointNetBn if bn else SuperPointNet)(max_keypoints=keypoints, keypoint_threshold=0.005)
    extractor.load_state_dict(syn.make_superpoint_state_dict(bn, seed=1))
    extractor = extractor.to(dev).train()                                  # finetune: True
    cfg = syn.make_config(descriptor_dim=256, num_stages=stages, num_heads=4, num_iters=20, side_info_size=1)
    model = SuperGlue(cfg)
    model.load_state_dict(syn.make_state_dict(cfg, seed=0))
    model = model.to(dev).train()
    opt = optim.Adam(list(model.parameters()) + list(extractor.parameters()), lr=lr, max_grad_norm=MAX_GRAD_NORM, scheduler_gamma=GAMMA)
    gen = torch.Generator(device=dev).manual_seed(seed)
    transform = augment.get_augmentation_transform({"name": augmentation})
    history = []
    for s in range(steps):
        if not fresh:
            gen.manual_seed(seed)
        item = augment.augment(pairs.homography_pairs(frames, offset, generator=gen), transform, gen)
        batch = extract(extractor, item)                                    # with grad: scores and descriptors carry a grad_fn
        opt.zero_grad(set_to_none=False)
        out = training_step(model, batch, MARGIN, with_labels=True)
        if out is None:
            log(f"step {s:2d}  no keypoints, skipped")
            continue
        total, lo, y_true = out
        total.backward()
        g1a = float(extractor.conv1a.weight.grad.abs().max())
        opt.step()
        matched = int((y_true["gt_matches0"] >= 0).sum())
        history.append((matched, float(total.detach()), g1a))
        log(f"step {s:2d}  keypoints {batch['lafs0'].shape[1]} / {batch['lafs1'].shape[1]} per image  matched labels {matched}  "
            f"loss {history[-1][1]:.4f}  nll {float(lo['loss']):.4f}  metric {float(lo['metric_loss']):.4f}  max|d loss / d conv1a.weight| {g1a:.3e}")
    return history


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--pairs", type=int, default=2)
    ap.add_argument("--size", type=int, nargs=2, default=(240, 320), metavar=("H", "W"))
    ap.add_argument("--offset", type=int, default=24)
    ap.add_argument("--keypoints", type=int, default=256)
    ap.add_argument("--lr", type=float, default=1e-4)
    ap.add_argument("--fresh", action="store_true")
    ap.add_argument("--bn", action="store_true", help="fine-tune SuperPointNetBn (train-mode BatchNorm)")
    ap.add_argument("--augment", default="none", choices=("none", "weak_color_aug"))
    a = ap.parse_args()
    run(a.steps, a.pairs, tuple(a.size), a.offset, a.keypoints, lr=a.lr, fresh=a.fresh, bn=a.bn, augmentation=a.augment)
