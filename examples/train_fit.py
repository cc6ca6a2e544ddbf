#!/usr/bin/env python3
"""The reference's whole training iteration on openglue_amd, optimizer included (models/matching_module.py:70-105 training_step,
:133-147 configure_optimizers, train.py:73 gradient_clip_val):

    supervision.generate_gt_matches -> SuperGlue(config).train()(data) -> supervision.criterion -> backward
    -> openglue_amd.optim.Adam(max_grad_norm=10, lr=1e-4, scheduler_gamma=0.999994).step()

The optimizer step is three HIP launches (gradient norm, scalars of the step, clip + Adam + StepLR + gradient reset) instead of
torch's foreach chain; the gradients are views into its flat buffer and come back zeroed.  --torch runs the same loop under
torch.nn.utils.clip_grad_norm_ + torch.optim.Adam + StepLR for comparison.  examples/train_step.py has the pairs and the step itself.

    python examples/train_fit.py [--steps 20] [--pairs 2] [--kpts 512] [--transform perspective|3d_reprojection] [--torch]"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from examples.train_step import MARGIN, make_pairs, training_step      # noqa: E402
from openglue_amd import optim, synthetic as syn                       # noqa: E402
from openglue_amd.superglue import SuperGlue                           # noqa: E402

MAX_GRAD_NORM, LR, GAMMA = 10.0, 1e-4, 0.999994


def run(steps=20, pairs=2, kpts=512, dim=128, stages=3, lr=LR, gamma=GAMMA, max_grad_norm=MAX_GRAD_NORM, transform="perspective",
        margin=MARGIN, use_torch=False, log=print):
    """`steps` iterations on one synthetic batch -> (total losses, gradients of the first step by parameter name, the model, the
    optimizer, parameters after the first step by name)"""
    dev = torch.device("cuda:0")
    cfg = syn.make_config(descriptor_dim=dim, num_stages=stages, num_heads=4, num_iters=20, side_info_size=1)
    model = SuperGlue(cfg)
    model.load_state_dict(syn.make_state_dict(cfg, seed=0))
    model = model.to(dev).train()
    if use_torch:
        opt = torch.optim.Adam(model.parameters(), lr=lr)
        sched = torch.optim.lr_scheduler.StepLR(opt, step_size=1, gamma=gamma)
    else:
        opt = optim.Adam(model.parameters(), lr=lr, max_grad_norm=max_grad_norm, scheduler_gamma=gamma)
    batch = make_pairs(pairs, kpts, dim, transform, dev)
    losses, first_grads, after_first = [], None, None
    t0 = time.perf_counter()
    for s in range(steps):
        opt.zero_grad(set_to_none=False)
        total, lo = training_step(model, batch, margin)
        total.backward()
        if first_grads is None:
            first_grads = {k: (None if p.grad is None else p.grad.detach().clone()) for k, p in model.named_parameters()}
        if use_torch:
            torch.nn.utils.clip_grad_norm_(model.parameters(), max_grad_norm)
            opt.step()
            sched.step()
        else:
            opt.step()
        if after_first is None:
            after_first = {k: p.detach().clone() for k, p in model.named_parameters()}
        losses.append(float(total.item()))
        if s % 5 == 0 or s + 1 == steps:
            log(f"step {s:3d}  total {losses[-1]:.4f}  nll {lo['loss'].item():.4f}  metric {lo['metric_loss'].item():.4f}")
    torch.cuda.synchronize(dev)
    log(f"{steps} steps of {pairs} pairs x {kpts} keypoints ({transform}) under {'torch.optim.Adam + clip_grad_norm_ + StepLR' if use_torch else 'openglue_amd.optim.Adam'}: "
        f"{(time.perf_counter() - t0) / steps * 1e3:.1f} ms per step incl. the loss read-back")
    return losses, first_grads, model, opt, after_first


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--pairs", type=int, default=2)
    ap.add_argument("--kpts", type=int, default=512)
    ap.add_argument("--transform", default="perspective", choices=("perspective", "3d_reprojection"))
    ap.add_argument("--torch", action="store_true", help="torch.optim.Adam + clip_grad_norm_ + StepLR instead of the fused step")
    a = ap.parse_args()
    run(a.steps, a.pairs, a.kpts, transform=a.transform, use_torch=a.torch)
