#!/usr/bin/env python3
"""The reference's validation step on openglue_amd (models/matching_module.py:107-131 validation_step + on_validation_epoch_end):

    SuperGlue.match(batch)                                 -> matches0 per keypoint of image 0
    AccuracyUsingEpipolarDist.update_batch(...)            -> per-pair precision / matching score (epipolar distance under E)
    CameraPoseAUC.update_batch(...)                        -> per-pair pose error (five-point RANSAC + cheirality)
    compute(), reset()                                     at the end of the epoch

on synthetic '3d_reprojection' pairs from examples/train_step.py.  Their baseline is small (|T| ~ 0.17 at depths 4-5, a few
pixels of parallax under 0.7 px of jitter), so even correct matches leave the translation direction uncertain by degrees: the
ground-truth line shows precision 1 with a pose AUC well below 1.  It prints the metrics of the model's matches and of the
ground-truth labels of supervision.generate_gt_matches (apply_thresholds=True): the latter is the sanity line for precision (~1).

    python examples/validate.py [--batches 4] [--pairs 4] [--kpts 1024]"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from examples.train_step import NEG_THR, POS_THR, make_pairs           # noqa: E402
from openglue_amd import features, metrics, supervision, synthetic as syn   # noqa: E402
from openglue_amd.superglue import SuperGlue                           # noqa: E402

# config/config.yaml evaluation: epipolar distance threshold, AUC thresholds (degrees), RANSAC threshold (pixels)
EPI_THR, AUC_THR, RANSAC_THR = 5e-4, [5.0, 10.0, 20.0], 1.0


def run(batches=4, pairs=4, kpts=1024, dim=128, log=print):
    dev = torch.device("cuda:0")
    cfg = syn.make_config(descriptor_dim=dim, num_stages=3, num_heads=4, num_iters=20, side_info_size=1)
    model = SuperGlue(cfg)
    model.load_state_dict(syn.make_state_dict(cfg, seed=0))
    model = model.to(dev).eval()
    sets = {name: (metrics.AccuracyUsingEpipolarDist(EPI_THR), metrics.CameraPoseAUC(AUC_THR, RANSAC_THR))
            for name in ("model", "ground truth")}
    for i in range(batches):
        batch = make_pairs(pairs, kpts, dim, "3d_reprojection", dev, seed=100 + i)
        f0 = features.prepare_features_output(batch["lafs0"], batch["scores0"], batch["descriptors0"], "none")
        f1 = features.prepare_features_output(batch["lafs1"], batch["scores1"], batch["descriptors1"], "none")
        data, y = supervision.generate_gt_matches(batch, f0, f1, POS_THR, NEG_THR, apply_thresholds=True)
        with torch.no_grad():
            pred = model.match(data, 0.2)
        tr = batch["transformation"]
        for name, m0 in (("model", pred["matches0"]), ("ground truth", y["gt_matches0"])):
            for metric in sets[name]:
                metric.update_batch(data["keypoints0"], data["keypoints1"], m0, tr)
    out = {}
    for name, (acc, auc) in sets.items():
        vals = {**acc.compute(), **auc.compute()}
        out[name] = {k: float(v) for k, v in vals.items()}
        log(f"{name:>12}: " + "  ".join(f"{k} {v:.4f}" for k, v in out[name].items()))
        acc.reset()
        auc.reset()
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=4)
    ap.add_argument("--pairs", type=int, default=4)
    ap.add_argument("--kpts", type=int, default=1024)
    a = ap.parse_args()
    run(a.batches, a.pairs, a.kpts)
