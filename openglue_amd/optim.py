"""The reference's optimizer step on HIP kernels: gradient clipping + Adam + StepLR in three launches.

The reference trains with torch.optim.Adam(lr=1e-4) and StepLR(step_size=1, gamma=0.999994) stepped every iteration
(models/matching_module.py:133-147) under Lightning's gradient_clip_val (train.py:73 = torch.nn.utils.clip_grad_norm_).  On the ~270
parameter tensors of the model that is a chain of foreach launches plus the norm / clamp / multiply launches of the clipping.  `Adam`
below does the same arithmetic through og_adam_step (csrc/optimizer.hip): one pass for the gradient norm, one single-workgroup kernel
for the scalars of the step, one pass that clips, updates p / exp_avg / exp_avg_sq and zeroes the gradient.

    opt = Adam(model.parameters(), lr=1e-4, max_grad_norm=10.0, scheduler_gamma=0.999994)
    loss.backward(); opt.step(); opt.zero_grad()

How it differs from torch.optim.Adam for the caller:
  * The optimizer owns three flat fp32 buffers (grad, exp_avg, exp_avg_sq).  Every `p.grad` is a VIEW into the flat gradient buffer;
    autograd accumulates in place into an existing `.grad`, so backward writes straight into it.  step() leaves the gradients zeroed
    and zero_grad() keeps the views (whatever `set_to_none` says): no memset, no re-allocation.  A caller that drops the views anyway
    (`model.zero_grad()` sets `.grad = None`) gets them back at the next step(): a missing gradient counts as zero, a foreign one is
    copied into the view (one extra device copy for that parameter).
  * Every parameter takes part in every step.  A zero gradient is a gradient, as under torch with zero_grad(set_to_none=False): the
    moments decay and the parameter moves by the decayed first moment.  torch skips parameters whose `.grad` is None; this class has
    no such state.
  * The effective learning rate is param_groups[0]['lr'] * scheduler_gamma ** (step - 1).  Either keep `lr` fixed and give
    scheduler_gamma (the built-in schedule: nothing runs on the host), or leave scheduler_gamma at 1 and attach a torch scheduler that
    rewrites `lr` (StepLR, Lightning's) -- not both, or the decay is applied twice.
  * The step count lives on the device; step() neither synchronises nor copies anything to the device.  `grad_norm` is a 0-d float64
    DEVICE tensor with the norm of the last step's gradients before clipping (what clip_grad_norm_ returns; NaN without max_grad_norm);
    the optimizer never reads it on the host.
  * The parameters are updated through raw pointers, so step() bumps every parameter's version counter itself
    (torch.autograd.graph.increment_version): SuperGlue's packed-weight cache and autograd's saved-tensor checks see the update.
  * state_dict() / load_state_dict() use torch.optim.Adam's format (per-parameter `step`, `exp_avg`, `exp_avg_sq`; torch's param_group
    keys): a Lightning checkpoint's optimizer_states[0] loads into this class, and what this class saves loads into torch.optim.Adam.
    max_grad_norm and scheduler_gamma are constructor arguments, not checkpoint state (as gradient_clip_val is the Trainer's).
Everything the reference does not use is refused with ValueError: several parameter groups, weight_decay, amsgrad, maximize,
parameters that are not contiguous fp32 tensors on one GPU.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib

_TORCH_ADAM_KEYS = ("foreach", "capturable", "differentiable", "fused", "decoupled_weight_decay")


class Adam(torch.optim.Optimizer):
    def __init__(self, params, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, max_grad_norm=None, scheduler_gamma=1.0):
        if not 0.0 <= lr:
            raise ValueError(f"Invalid learning rate: {lr}")
        if not 0.0 <= eps:
            raise ValueError(f"Invalid epsilon value: {eps}")
        if not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0):
            raise ValueError(f"Invalid beta parameters: {betas}")
        if max_grad_norm is not None and not max_grad_norm > 0.0:
            raise ValueError(f"Invalid max_grad_norm: {max_grad_norm}")
        if not 0.0 < scheduler_gamma <= 1.0:
            raise ValueError(f"Invalid scheduler_gamma: {scheduler_gamma}")
        # torch.optim.Adam's keys, so that param_groups travel between the two classes; the values are the only ones supported
        defaults = dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=0, amsgrad=False, maximize=False)
        defaults.update({k: v for k, v in torch.optim.Adam([torch.zeros(1)]).defaults.items() if k in _TORCH_ADAM_KEYS})
        super().__init__(params, defaults)
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.scheduler_gamma = float(scheduler_gamma)
        self._check_groups()
        self._params = list(self.param_groups[0]["params"])
        for i, p in enumerate(self._params):
            if p.dtype != torch.float32:
                raise ValueError(f"parameter {i}: {p.dtype}; only float32 parameters are supported")
            if not p.is_contiguous():
                raise ValueError(f"parameter {i}: not contiguous")
            if not p.is_cuda:
                raise ValueError(f"parameter {i}: on {p.device}; openglue_amd.optim.Adam has no CPU path")
            if p.device != self._params[0].device:
                raise ValueError(f"parameter {i}: on {p.device}, parameter 0 on {self._params[0].device}; one device only")
            if p.numel() == 0:
                raise ValueError(f"parameter {i}: empty")
        self._device = self._params[0].device
        self._build()

    # ------------------------------------------------------------------ layout
    def _check_groups(self):
        if len(self.param_groups) != 1:
            raise ValueError(f"{len(self.param_groups)} parameter groups; openglue_amd.optim.Adam supports one (the reference uses one)")
        g = self.param_groups[0]
        if g.get("weight_decay", 0) != 0:
            raise ValueError("weight_decay != 0 is not supported (the reference uses none)")
        for key in ("amsgrad", "maximize"):
            if g.get(key, False):
                raise ValueError(f"{key}=True is not supported (the reference does not use it)")

    def _build(self):
        """Flat buffers, device table and chunk map: once; the table again when a parameter's storage moved."""
        dev, n = self._device, len(self._params)
        lib = _lib.load()
        numel = (C.c_int64 * n)(*[p.numel() for p in self._params])
        offsets = (C.c_int64 * n)()
        lay = _lib.og_adam_layout_t()
        _lib.check(lib.og_adam_layout(n, numel, offsets, None, C.byref(lay)), "og_adam_layout")
        cmap = (C.c_int32 * (2 * lay.num_chunks))()
        _lib.check(lib.og_adam_layout(n, numel, offsets, cmap, C.byref(lay)), "og_adam_layout")
        self._layout, self._offsets = lay, list(offsets)
        self._flat_grad = torch.zeros(lay.total, device=dev, dtype=torch.float32)
        self._exp_avg = torch.zeros(lay.total, device=dev, dtype=torch.float32)
        self._exp_avg_sq = torch.zeros(lay.total, device=dev, dtype=torch.float32)
        self._workspace = torch.zeros(lay.workspace_bytes // 8, device=dev, dtype=torch.float64)      # scalars block (step = 0) + norm partials
        self.grad_norm = self._workspace[_lib.OG_ADAM_TOTAL_NORM]
        self._chunk_map = torch.tensor(list(cmap), dtype=torch.int32).to(dev)
        self._grad_views = [self._view(self._flat_grad, i) for i in range(n)]
        for p, gv in zip(self._params, self._grad_views):
            if p.grad is not None:
                gv.copy_(p.grad)
            p.grad = gv
        self._build_table()
        self._clean_version = -1                    # gradients taken over from the caller count as accumulated

    def _view(self, flat, i):
        p = self._params[i]
        return flat[self._offsets[i]: self._offsets[i] + p.numel()].view(p.shape)

    def _build_table(self):
        self._ptrs = [p.data_ptr() for p in self._params]
        self._ptr_array = (C.c_void_p * len(self._ptrs))(*self._ptrs)
        rows = [[ptr, off, p.numel()] for ptr, off, p in zip(self._ptrs, self._offsets, self._params)]
        self._table = torch.tensor(rows, dtype=torch.int64).to(self._device)

    # ------------------------------------------------------------------ the step
    def zero_grad(self, set_to_none: bool = True):
        """The gradients are views into the flat buffer and are kept, whatever `set_to_none` says.  After step() they are already zero
        (the update kernel wrote the zeros) and nothing is launched; gradients accumulated since then -- a step the caller skipped --
        are cleared: autograd's in-place accumulation shows in the buffer's version counter, the kernel's raw stores do not."""
        if self._flat_grad._version != self._clean_version:
            self._flat_grad.zero_()
            self._clean_version = self._flat_grad._version

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        g = self.param_groups[0]
        self._check_groups()
        moved = False
        for i, p in enumerate(self._params):
            if p.device != self._device:
                raise RuntimeError(f"parameter {i} moved from {self._device} to {p.device} after the optimizer was built; build a new optimizer")
            if p.data_ptr() != self._ptrs[i]:
                moved = True
            gv = self._grad_views[i]
            if p.grad is not gv:                    # the caller dropped or replaced the view
                if p.grad is not None:
                    gv.copy_(p.grad)
                p.grad = gv
        if moved:
            self._build_table()
        lay = self._layout
        clip = self.max_grad_norm is not None
        _lib.call("og_adam_step", self._device, len(self._params), self._ptr_array, self._table.data_ptr(), self._chunk_map.data_ptr(),
                  lay.num_chunks, lay.total, self._flat_grad.data_ptr(), self._exp_avg.data_ptr(), self._exp_avg_sq.data_ptr(),
                  self._workspace.data_ptr(), float(g["lr"]), self.scheduler_gamma, float(g["betas"][0]), float(g["betas"][1]),
                  float(g["eps"]), int(clip), self.max_grad_norm if clip else 0.0, _lib.STREAM)
        torch.autograd.graph.increment_version(self._params)       # the kernels wrote through raw pointers
        self._clean_version = self._flat_grad._version
        return loss

    # ------------------------------------------------------------------ checkpoints (torch.optim.Adam's format)
    def state_dict(self):
        step = self._workspace[_lib.OG_ADAM_STEP].to(dtype=torch.float32, device="cpu")      # the one host read: checkpoints only
        self.state.clear()
        if float(step) > 0:
            for i, p in enumerate(self._params):
                self.state[p] = {"step": step.clone(), "exp_avg": self._view(self._exp_avg, i).clone(),
                                 "exp_avg_sq": self._view(self._exp_avg_sq, i).clone()}
        try:
            return super().state_dict()
        finally:
            self.state.clear()

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)         # checks the group / parameter counts, casts the state to the parameters' device
        self._check_groups()
        new = self.param_groups[0]["params"]
        if len(new) != len(self._params) or any(a is not b for a, b in zip(new, self._params)):
            raise ValueError("load_state_dict changed the parameter list")
        steps = set()
        for i, p in enumerate(self._params):
            st = self.state.get(p)
            if not st:
                steps.add(0.0)
                self._view(self._exp_avg, i).zero_()
                self._view(self._exp_avg_sq, i).zero_()
                continue
            if "max_exp_avg_sq" in st:
                raise ValueError("the checkpoint holds amsgrad state; amsgrad is not supported")
            steps.add(float(st["step"]))
            self._view(self._exp_avg, i).copy_(st["exp_avg"])
            self._view(self._exp_avg_sq, i).copy_(st["exp_avg_sq"])
        if len(steps) != 1:
            raise ValueError(f"the parameters of the checkpoint are at different steps {sorted(steps)}; this optimizer keeps one step count")
        self._workspace[_lib.OG_ADAM_STEP] = steps.pop()
        self.state.clear()                          # the flat buffers are the state
