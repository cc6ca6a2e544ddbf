#!/usr/bin/env python3
"""Time the optimizer step of the reference's training loop on the C2 model's parameter set (256-d, 9 stages: 11,957,249 parameters):

    torch:  zero_grad(set_to_none=False), clip_grad_norm_(10), torch.optim.Adam.step (its default implementation), StepLR.step
    fused:  openglue_amd.optim.Adam(max_grad_norm=10, scheduler_gamma=0.999994): step + zero_grad (three launches)

Both run in one process, alternating, three repeats each; device events around STEPS steps after WARMUP steps; the gradients are
refilled by a device copy outside the timed window (and, inside it, simply stay zero: both steps do the same work on zeros).  Also
the launches per step of each (kernel_trace.launched_kernels), the algorithmic bytes -- read p, g, m, v and write p, g, m, v = 32 B
per parameter -- as a share of the 8 TB/s HBM peak, and the C2-sized training step (4 pairs x 1024 keypoints, as
scripts/bench_train_step.py) under each optimizer.  Needs an MI355X: without a GPU it fails.

    python scripts/bench_optimizer.py            # STEPS=200 WARMUP=20 REPEATS=3 TRAIN_STEPS=5 (environment)"""
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from openglue_amd import kernel_trace, optim, synthetic as syn      # noqa: E402
from openglue_amd.superglue import SuperGlue                        # noqa: E402
from oracle import superglue_oracle as orc                          # noqa: E402  (only nll_criterion, as scripts/bench_train_step.py)

STEPS = int(os.environ.get("STEPS", 200)); WARMUP = int(os.environ.get("WARMUP", 20)); REPEATS = int(os.environ.get("REPEATS", 3))
TRAIN_STEPS = int(os.environ.get("TRAIN_STEPS", 5))
MAX_NORM, LR, GAMMA = 10.0, 1e-4, 0.999994
HBM_PEAK = 8e12

if not torch.cuda.is_available():
    sys.exit("bench_optimizer.py needs an MI355X: no GPU is visible (there is no CPU path to fall back to)")
dev = torch.device("cuda:0")
cfg = syn.make_config(descriptor_dim=256, num_stages=9, num_heads=4, num_iters=20)


def model_on_gpu():
    model = SuperGlue(cfg)
    model.load_state_dict(syn.make_state_dict(cfg, seed=0))
    return model.to(dev).train()


def make(kind, params):
    """-> (optimizer, step function with everything the loop runs per iteration for the optimizer)"""
    if kind == "torch":
        opt = torch.optim.Adam(params, lr=LR)
        sched = torch.optim.lr_scheduler.StepLR(opt, step_size=1, gamma=GAMMA)

        def step():
            torch.nn.utils.clip_grad_norm_(params, MAX_NORM)
            opt.step()
            sched.step()
            opt.zero_grad(set_to_none=False)
    else:
        opt = optim.Adam(params, lr=LR, max_grad_norm=MAX_NORM, scheduler_gamma=GAMMA)

        def step():
            opt.step()
            opt.zero_grad()
    return opt, step


def timed(step, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        step()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / n


# ---------------------------------------------------------------------------------------- the step alone
sets, steps, source = {}, {}, {}
for kind in ("torch", "fused"):
    params = [p for p in model_on_gpu().parameters()]
    g = torch.Generator(device=dev).manual_seed(0)
    source[kind] = [1e-3 * torch.randn(p.shape, device=dev, generator=g) for p in params]
    sets[kind] = params
    _, steps[kind] = make(kind, params)
numel = sum(p.numel() for p in sets["torch"])


def refill(kind):
    for p, s in zip(sets[kind], source[kind]):
        if p.grad is None:
            p.grad = s.clone()
        else:
            p.grad.copy_(s)


launches = {}
for kind in ("torch", "fused"):
    refill(kind)
    steps[kind]()                                   # state initialisation of torch's Adam happens here
    refill(kind)
    launches[kind] = kernel_trace.launched_kernels(steps[kind])
ms = {"torch": [], "fused": []}
for r in range(REPEATS):
    for kind in ("torch", "fused"):
        refill(kind)
        timed(steps[kind], WARMUP)
        refill(kind)
        torch.cuda.synchronize()
        ms[kind].append(timed(steps[kind], STEPS))
bytes_algo = 32 * numel
print(f"optimizer step on {numel} parameters in {len(sets['torch'])} tensors, {STEPS} steps after {WARMUP} warm-up, {REPEATS} repeats, alternating")
for kind in ("torch", "fused"):
    med = statistics.median(ms[kind])
    print(f"  {kind:5s}: {med:.4f} ms per step (repeats {' '.join(f'{v:.4f}' for v in ms[kind])}); {len(launches[kind])} launches per step; "
          f"{bytes_algo / 1e6:.0f} MB algorithmic = {bytes_algo / (med * 1e-3) / 1e12:.2f} TB/s = {100 * bytes_algo / (med * 1e-3) / HBM_PEAK:.0f} % of the 8 TB/s HBM peak "
          f"(bound {bytes_algo / HBM_PEAK * 1e6:.0f} us)")
names = {}
for n in launches["torch"]:
    names[n.split("<")[0]] = names.get(n.split("<")[0], 0) + 1
print("  torch's launches by kernel: " + ", ".join(f"{v} x {k}" for k, v in sorted(names.items(), key=lambda kv: -kv[1])))
print("  fused launches: " + ", ".join(launches["fused"]))
spread = max(max(v) - min(v) for v in ms.values())
print(f"  fused / torch = {statistics.median(ms['fused']) / statistics.median(ms['torch']):.3f}; largest spread between repeats of one code {spread:.4f} ms")
del sets, steps, source
torch.cuda.empty_cache()

# ---------------------------------------------------------------------------------------- the C2-sized training step under each optimizer
B, N = 4, 1024
data = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in syn.make_batch(B, N, N, 256, 1, seed=1).items()}
gen = torch.Generator().manual_seed(0)
gt0 = torch.full((B, N), -1, dtype=torch.long); gt1 = torch.full((B, N), -1, dtype=torch.long)
for b in range(B):
    i = torch.randperm(N, generator=gen)[: N // 2]; j = torch.randperm(N, generator=gen)[: N // 2]
    gt0[b, i] = j; gt1[b, j] = i
gt0, gt1 = gt0.to(dev), gt1.to(dev)
train_ms = {"torch": [], "fused": []}
loops = {}
for kind in ("torch", "fused"):
    model = model_on_gpu()
    _, opt_step = make(kind, list(model.parameters()))

    def train_step(model=model, opt_step=opt_step):
        orc.nll_criterion(model(data)["scores"], gt0, gt1).backward()
        opt_step()
    loops[kind] = train_step
    train_step(); train_step()
    torch.cuda.synchronize()
for r in range(REPEATS):
    for kind in ("torch", "fused"):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(TRAIN_STEPS):
            loops[kind]()
        torch.cuda.synchronize()
        train_ms[kind].append((time.perf_counter() - t0) / TRAIN_STEPS * 1e3)
print(f"training step, C2 model, {B} pairs x {N} keypoints, 20 Sinkhorn iterations (forward + NLL + backward + optimizer), {TRAIN_STEPS} steps x {REPEATS} repeats:")
for kind in ("torch", "fused"):
    print(f"  under {kind:5s}: {statistics.median(train_ms[kind]):.2f} ms per step (repeats {' '.join(f'{v:.2f}' for v in train_ms[kind])})")
