#!/usr/bin/env python3
"""Criterion fixtures FROM THE REFERENCE on CPU (build container only: needs a checkout of the reference).

    python tests/golden/make_golden_criterion.py <reference checkout>      # writes tests/golden/criterion.npz

The reference's own criterion (utils/losses.py, imported unchanged) in fp32 on the seeded cases of tests/criterion_cases.py: the
seven regular cases and the three whose positive is the only entry of its row / column, each with margin None and 0.2.  Per
case and margin <name>_{none,margin}_*: loss, metric_loss and the gradients of 0.7 * loss + 1.9 * metric_loss by autograd
(grad_scores; grad_desc0 and grad_desc1 with a margin).  Results only: the tests rebuild the inputs from the same generator."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
if len(sys.argv) != 2:
    sys.exit(__doc__)
sys.path.insert(0, sys.argv[1])

from utils.losses import criterion                               # noqa: E402

from tests import criterion_cases as cc                          # noqa: E402


def record(out, name, case):
    S, A, Bd, gt0, gt1 = case
    for margin in (None, cc.MARGIN):
        key = f"{name}_{'none' if margin is None else 'margin'}"
        s_, a_, b_ = (t.clone().requires_grad_(True) for t in (S, A, Bd))
        lo = criterion({"gt_matches0": gt0, "gt_matches1": gt1}, {"scores": s_, "context_descriptors0": a_, "context_descriptors1": b_},
                       margin=margin)
        (cc.W_LOSS * lo["loss"] + cc.W_METRIC * lo["metric_loss"]).backward()
        out[f"{key}_loss"] = np.float32(lo["loss"].item())
        out[f"{key}_metric_loss"] = np.float32(lo["metric_loss"].item())
        out[f"{key}_grad_scores"] = s_.grad.numpy().copy()
        if margin is not None:
            out[f"{key}_grad_desc0"], out[f"{key}_grad_desc1"] = a_.grad.numpy().copy(), b_.grad.numpy().copy()
        print(key, "loss", lo["loss"].item(), "metric", lo["metric_loss"].item())


def main():
    out = {}
    for shape in cc.REGULAR:
        record(out, cc.case_name(shape), cc.regular_case(shape))
    for m, n in cc.SINGLE:
        record(out, f"single_m{m}_n{n}", cc.single_case(m, n))
    path = os.path.join(HERE, "criterion.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
