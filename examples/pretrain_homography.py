#!/usr/bin/env python3
"""The reference's first training stage -- self-supervised homography pre-training (pretrain_homography.py,
config/homography_pretraining.yaml, data/oxford_paris_dataset.py) -- from images, on openglue_amd:

    uint8 frames --pairs.homography_pairs-->  image0, image1, H      (random corner displacements drawn on the device)
    --augment weak_color_aug: augment.augment on image0, image1    (equalize, sharpness, solarize, noise; every sample its own draw)
    SIFT (or --features superpoint) on both views                 -> LAFs, responses, descriptors
    examples/train_step.py training_step: prepare_features_output -> generate_gt_matches -> SuperGlue.train() -> criterion
    backward -> openglue_amd.optim.Adam (clip + Adam + StepLR), the constants of examples/train_fit.py

The frames are synthetic (synthetic.make_image, three grey renderings as R, G, B) and stand for what a loader hands over after
decoding and resizing.  From there to the parameter update every tensor stays on the GPU: nothing is copied to the host between the
frames and the optimizer step except the extractor's own keypoint count (one integer per image batch) and the numbers printed here.
A fresh pair is synthesised from the same frames every step, as a data loader would.

--validate adds what the reference's stage lacks (its data module has a train_dataloader only and it trains with
num_sanity_val_steps=0): after the last step the model goes to eval(), fresh pairs from the same frames go through the extractor and
SuperGlue.match, and metrics.HomographyAccuracy / metrics.HomographyAUC judge the matches against the pairs' own H: precision and
matching score at 3 px, and the AUC of the mean corner error of a homography estimated from the matches (geometry.homography).

    python examples/pretrain_homography.py [--steps 5] [--pairs 2] [--size 240 320] [--offset 24] [--features sift|superpoint]
                                         [--augment none|weak_color_aug] [--validate]"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from examples.train_fit import GAMMA, LR, MAX_GRAD_NORM                # noqa: E402
from examples.train_step import MARGIN, training_step                  # noqa: E402
from openglue_amd import augment, features, metrics, optim, pairs, synthetic as syn       # noqa: E402
from openglue_amd.sift import SIFT                                     # noqa: E402
from openglue_amd.superglue import SuperGlue                           # noqa: E402
from openglue_amd.superpoint import SuperPointNetBn                    # noqa: E402


def make_frames(B, H, W, dev, seed=0):
    """[B, H, W, 3] uint8 on the device"""
    rgb = torch.stack([torch.cat([syn.make_image(H, W, seed=seed + 3 * b + c)[0] for c in range(3)]) for b in range(B)])
    return (rgb * 255).round().to(torch.uint8).permute(0, 2, 3, 1).contiguous().to(dev)


def make_extractor(name, keypoints, dev):
    if name == "sift":
        return SIFT(max_keypoints=keypoints), 128
    sp = SuperPointNetBn(max_keypoints=keypoints, keypoint_threshold=0.005)
    sp.load_state_dict(syn.make_superpoint_state_dict(True, seed=1))
    return sp.eval().to(dev), 256


def extract(extractor, item):
    """the pair item -> the batch examples/train_step.py's training_step takes (cached-features layout)"""
    batch = {"transformation": item["transformation"]}
    for side in "01":
        image = item["image" + side]
        lafs, scores, desc = extractor(image)
        batch.update({"lafs" + side: lafs, "scores" + side: scores, "descriptors" + side: desc,
                      f"image{side}_size": [image.shape[3], image.shape[2]]})
    return batch


VAL_THRESHOLD = 3.0                 # pixels: a correct match, and the RANSAC inlier threshold
VAL_AUC_THRESHOLDS = (3, 5, 10)     # pixels of mean corner error


def validate(model, extractor, frames, offset, gen, batches=2, match_threshold=0.2, log=print):
    """`batches` fresh pair batches through eval() -> SuperGlue.match -> HomographyAccuracy and HomographyAUC.  Leaves the model in
    eval().  -> {'Precision', 'Matching Score', 'AUC@3px', 'AUC@5px', 'AUC@10px'} as floats"""
    model.eval()
    h, w = frames.shape[1] - 2 * offset, frames.shape[2] - 2 * offset
    acc = metrics.HomographyAccuracy(VAL_THRESHOLD)
    auc = metrics.HomographyAUC(VAL_AUC_THRESHOLDS, VAL_THRESHOLD, (w, h))
    with torch.no_grad():
        for _ in range(batches):
            batch = extract(extractor, pairs.homography_pairs(frames, offset, generator=gen))
            if batch["lafs0"].shape[1] == 0 or batch["lafs1"].shape[1] == 0:
                continue
            f = [features.prepare_features_output(batch["lafs" + s], batch["scores" + s], batch["descriptors" + s], "none") for s in "01"]
            data = {"image0_size": batch["image0_size"], "image1_size": batch["image1_size"]}
            for s in "01":
                data.update({"keypoints" + s: f[int(s)]["keypoints"], "local_descriptors" + s: f[int(s)]["local_descriptors"],
                             "side_info" + s: f[int(s)]["side_info"]})
            out = model.match(data, match_threshold, both_sides=False)
            acc.update_batch(data["keypoints0"], data["keypoints1"], out["matches0"], batch["transformation"])
            auc.update_batch(data["keypoints0"], data["keypoints1"], out["matches0"], batch["transformation"])
    if not acc.precision:
        log("validation: no keypoints, nothing to judge")
        return {}
    result = {k: float(v) for k, v in {**acc.compute(), **auc.compute()}.items()}
    log("validation  " + "  ".join(f"{k} {v:.4f}" for k, v in result.items()))
    return result


def run(steps=5, n_pairs=2, size=(240, 320), offset=24, feature="sift", keypoints=512, stages=3, seed=0, log=print, augmentation="none",
        validation=False):
    """-> [(matched labels, total loss)] per step"""
    dev = torch.device("cuda:0")
    H, W = size
    frames = make_frames(n_pairs, H, W, dev, seed)
    extractor, dim = make_extractor(feature, keypoints, dev)
    cfg = syn.make_config(descriptor_dim=dim, num_stages=stages, num_heads=4, num_iters=20, side_info_size=1)
    model = SuperGlue(cfg)
    model.load_state_dict(syn.make_state_dict(cfg, seed=0))
    model = model.to(dev).train()
    opt = optim.Adam(model.parameters(), lr=LR, max_grad_norm=MAX_GRAD_NORM, scheduler_gamma=GAMMA)
    gen = torch.Generator(device=dev).manual_seed(seed)
    transform = augment.get_augmentation_transform({"name": augmentation})
    history = []
    for s in range(steps):
        item = augment.augment(pairs.homography_pairs(frames, offset, generator=gen), transform, gen)
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
            f"loss {history[-1][1]:.4f}  nll {float(lo['loss']):.4f}  metric {float(lo['metric_loss']):.4f}")
    if validation:
        validate(model, extractor, frames, offset, gen, log=log)
    return history


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--pairs", type=int, default=2)
    ap.add_argument("--size", type=int, nargs=2, default=(240, 320), metavar=("H", "W"))
    ap.add_argument("--offset", type=int, default=24)
    ap.add_argument("--features", default="sift", choices=("sift", "superpoint"))
    ap.add_argument("--keypoints", type=int, default=512)
    ap.add_argument("--augment", default="none", choices=("none", "weak_color_aug"))
    ap.add_argument("--validate", action="store_true", help="after training: precision, matching score and corner-error AUC on fresh pairs")
    a = ap.parse_args()
    run(a.steps, a.pairs, tuple(a.size), a.offset, a.features, a.keypoints, augmentation=a.augment, validation=a.validate)
