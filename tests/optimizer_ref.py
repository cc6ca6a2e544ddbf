"""Float64 restatement of the reference's optimizer step: torch.nn.utils.clip_grad_norm_ (Lightning's gradient_clip_val, train.py:73), then
torch.optim.Adam, under StepLR(step_size=1) stepped every iteration (models/matching_module.py:133-147).  The learning rate is written
in closed form, lr * gamma^(step-1), where StepLR multiplies step by step.  tests/test_optimizer_cpu.py holds it against torch's own
classes run in float64; the GPU tests use it as the exact answer the fp32 kernels (and torch's fp32 step) are measured against.

Also the parameter sets the optimizer tests share: shapes and seeded values of the SuperGlue configurations' learnable parameters."""
import math

import torch

from openglue_amd import synthetic as syn

LEARNABLE = ("conv_w", "conv_b", "bn_w", "bn_b", "mix", "dustbin")


class RefAdam:
    """params: float64 tensors, updated in place by step(grads).  A zero gradient is a gradient: every parameter moves every step."""

    def __init__(self, params, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, max_grad_norm=None, scheduler_gamma=1.0):
        assert all(p.dtype == torch.float64 for p in params)
        self.params = list(params)
        self.lr, self.betas, self.eps, self.max_grad_norm, self.gamma = float(lr), (float(betas[0]), float(betas[1])), float(eps), max_grad_norm, float(scheduler_gamma)
        self.exp_avg = [torch.zeros_like(p) for p in self.params]
        self.exp_avg_sq = [torch.zeros_like(p) for p in self.params]
        self.steps = 0
        self.grad_norm = None
        self.clip_coef = 1.0

    def step(self, grads, lr=None):
        """One step on float64 gradients (not modified).  lr overrides the base rate (a host-side scheduler's value)."""
        b1, b2 = self.betas
        total = math.sqrt(sum(float((g.double() ** 2).sum()) for g in grads))
        self.grad_norm = total
        self.clip_coef = 1.0 if self.max_grad_norm is None else min(1.0, self.max_grad_norm / (total + 1e-6))
        self.steps += 1
        t = self.steps
        lr_t = (self.lr if lr is None else lr) * self.gamma ** (t - 1)
        step_size = lr_t / (1.0 - b1 ** t)
        bc2_sqrt = math.sqrt(1.0 - b2 ** t)
        for p, g, m, v in zip(self.params, grads, self.exp_avg, self.exp_avg_sq):
            g = g.double() * self.clip_coef
            m.add_((g - m) * (1.0 - b1))
            v.mul_(b2).add_(g * g * (1.0 - b2))
            p.sub_(step_size * m / (v.sqrt() / bc2_sqrt + self.eps))
        return total


def rel_err(got, want) -> float:
    """max |got - want| / max |want| over every element of two lists of tensors (or two tensors), in float64"""
    if torch.is_tensor(got):
        got, want = [got], [want]
    num = max(float((a.detach().double().cpu() - b.double()).abs().max()) for a, b in zip(got, want))
    return num / max(float(b.double().abs().max()) for b in want)


def config(name):
    return syn.make_config(**{k: v for k, v in syn.CONFIGS[name].items() if k not in ("kpts", "batch")})


def parameter_set(name, seed=0):
    """[(name, float32 tensor)] of the learnable parameters of BASELINE config `name`, in registration order, with seeded values"""
    cfg = config(name)
    spec = syn.state_dict_spec(cfg)
    sd = syn.make_state_dict(cfg, seed=seed)
    return [(k, sd[k].float().clone()) for k, (_, kind, _) in spec.items() if kind in LEARNABLE]


def parameter_numels(name):
    cfg = config(name)
    return [max(1, math.prod(shape)) for shape, kind, _ in syn.state_dict_spec(cfg).values() if kind in LEARNABLE]


def gradient_scales(steps, numel, seed=0, max_norm=10.0):
    """Per step, the factor that gives a standard-normal gradient of `numel` elements a norm below max_norm (about half of the steps:
    0.57 .. 0.9 of it) or above it (up to 570 times): clipped and unclipped steps both occur"""
    g = torch.Generator().manual_seed(1000 + seed)
    u = torch.rand(steps, 2, generator=g, dtype=torch.float64)
    target = torch.where(u[:, 0] < 0.5, max_norm * (0.57 + 0.33 * u[:, 1]), max_norm * 10.0 ** (0.1 + 2.65 * u[:, 1]))
    return (target / math.sqrt(numel)).tolist()
