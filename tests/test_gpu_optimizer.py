"""GPU: the fused clip + Adam + StepLR step (openglue_amd.optim.Adam over og_adam_step, csrc/optimizer.hip) against the float64
restatement of tests/optimizer_ref.py.

The parity bar is relative to torch itself: in the same test torch's own fp32 step (clip_grad_norm_ + torch.optim.Adam + StepLR on the
CPU) runs on the same inputs, and its error against float64 is measured the same way (max |x - x64| / max |x64| over all elements of
the parameters, of exp_avg and of exp_avg_sq).  The kernels may be at most 4 times as far from float64 as torch is: they evaluate the
same fp32 expressions, and the factor covers what torch's run does not share -- the order of the norm's summation (hence the last bit
of the clip coefficient), a reciprocal multiply where torch divides by sqrt(bias_correction2), and fused multiply-adds."""
import math

import numpy as np
import pytest
import torch

from openglue_amd import kernel_trace, synthetic as syn
from tests import optimizer_ref as ref
from tests.util import parity_note

pytestmark = pytest.mark.gpu

MAX_NORM = 10.0
BAR = 4.0


def _torch_cpu_and_ref(init, grads_per_step, lr, gamma, max_norm=MAX_NORM):
    """torch's fp32 step on the CPU and the float64 restatement over the same fp32 gradients -> (RefAdam, torch parameters, torch
    optimizer, norms per step, clipped steps)"""
    params = [torch.nn.Parameter(t.clone()) for t in init]
    opt = torch.optim.Adam(params, lr=lr)
    sched = torch.optim.lr_scheduler.StepLR(opt, step_size=1, gamma=gamma)
    exact = ref.RefAdam([t.double().clone() for t in init], lr=lr, max_grad_norm=max_norm, scheduler_gamma=gamma)
    norms, clipped = [], 0
    for grads in grads_per_step:
        for p, g in zip(params, grads):
            p.grad = g.clone()
        torch.nn.utils.clip_grad_norm_(params, max_norm)
        opt.step()
        sched.step()
        norms.append(exact.step(grads))
        clipped += exact.clip_coef < 1.0
    return exact, params, opt, norms, clipped


def _errors(exact, params, exp_avg, exp_avg_sq):
    return (ref.rel_err([p.detach() for p in params], exact.params), ref.rel_err(exp_avg, exact.exp_avg), ref.rel_err(exp_avg_sq, exact.exp_avg_sq))


def _torch_errors(exact, params, opt):
    return _errors(exact, params, [opt.state[p]["exp_avg"] for p in params], [opt.state[p]["exp_avg_sq"] for p in params])


def _our_errors(exact, params, opt):
    st = opt.state_dict()["state"]
    return _errors(exact, params, [st[i]["exp_avg"] for i in range(len(params))], [st[i]["exp_avg_sq"] for i in range(len(params))])


def _grads(init, steps, seed):
    """seeded fp32 gradients per step whose norm lies below MAX_NORM on about half of the steps and up to 570 times above it on the others"""
    g = torch.Generator().manual_seed(seed)
    numel = sum(t.numel() for t in init)
    return [[s * torch.randn(t.shape, generator=g) for t in init] for s in ref.gradient_scales(steps, numel, seed=seed, max_norm=MAX_NORM)]


def _set_grads(params, grads):
    for p, g in zip(params, grads):
        if p.grad is None:
            p.grad = g.to(p.device)
        else:
            p.grad.copy_(g)


def _assert_within_bar(what, ours, torchs):
    parity_note(f"optimizer {what}: error against float64 of (param, exp_avg, exp_avg_sq) ours " + " ".join(f"{e:.3e}" for e in ours)
                + " torch-fp32 " + " ".join(f"{e:.3e}" for e in torchs))
    for name, a, b in zip(("param", "exp_avg", "exp_avg_sq"), ours, torchs):
        assert b > 0 and a <= BAR * b, (what, name, a, b)


def test_parity_with_float64_on_the_c2_parameter_set(gpu_device):
    """50 steps on parameters with the C2 state-dict's shapes (11,957,249 elements; dustbin_score has one element, so
    the scalar tail runs), seeded gradients, clipped and unclipped steps mixed.  lr = 1e-3 and gamma = 0.97 instead of the reference's
    1e-4 and 0.999994, so that the schedule is visible at the bar: at the reference's values 50 steps of decay change the parameters by
    less than torch's own rounding error, and a wrong schedule would pass.  Recorded figures: see the parity note."""
    from openglue_amd.optim import Adam
    lr, gamma, steps = 1e-3, 0.97, 50
    init = [t for _, t in ref.parameter_set("C2", seed=0)]
    assert sum(t.numel() for t in init) == 11_957_249 and min(t.numel() for t in init) == 1
    params = [torch.nn.Parameter(t.to(gpu_device)) for t in init]
    opt = Adam(params, lr=lr, max_grad_norm=MAX_NORM, scheduler_gamma=gamma)
    # torch's run on the same list of tensors (its norm is a norm of per-tensor norms); the float64 restatement on one flat tensor:
    # the exact answer does not depend on the grouping, and it is far fewer calls
    flat = torch.cat([t.reshape(-1) for t in init])
    tparams = [torch.nn.Parameter(t.clone()) for t in init]
    topt = torch.optim.Adam(tparams, lr=lr)
    sched = torch.optim.lr_scheduler.StepLR(topt, step_size=1, gamma=gamma)
    exact = ref.RefAdam([flat.double()], lr=lr, max_grad_norm=MAX_NORM, scheduler_gamma=gamma)
    g = torch.Generator().manual_seed(11)
    sizes = [t.numel() for t in init]
    clipped, worst_norm = 0, 0.0
    for scale in ref.gradient_scales(steps, flat.numel(), seed=11, max_norm=MAX_NORM):
        gflat = scale * torch.randn(flat.numel(), generator=g)
        grads = [c.view(t.shape) for c, t in zip(gflat.split(sizes), init)]
        _set_grads(params, grads)
        opt.step()
        for p, gr in zip(tparams, grads):
            p.grad = gr.clone()
        torch.nn.utils.clip_grad_norm_(tparams, MAX_NORM)
        topt.step()
        sched.step()
        want = exact.step([gflat])
        clipped += exact.clip_coef < 1.0
        worst_norm = max(worst_norm, abs(float(opt.grad_norm) - want) / want)
    print(f"clipped {clipped} of {steps} steps; worst relative error of grad_norm {worst_norm:.3e}")
    assert clipped >= 10 and steps - clipped >= 10, clipped
    assert worst_norm < 1e-6, worst_norm
    st = opt.state_dict()["state"]
    cat = lambda ts: torch.cat([t.detach().reshape(-1).cpu() for t in ts])
    ours = _errors(exact, [cat(params)], [cat(st[i]["exp_avg"] for i in range(len(params)))], [cat(st[i]["exp_avg_sq"] for i in range(len(params)))])
    torchs = _errors(exact, [cat(tparams)], [cat(topt.state[p]["exp_avg"] for p in tparams)], [cat(topt.state[p]["exp_avg_sq"] for p in tparams)])
    _assert_within_bar(f"C2 x {steps} steps ({clipped} clipped)", ours, torchs)
    assert float(st[0]["step"]) == steps
    assert all(bool((p.grad == 0).all()) for p in params)


def test_two_runs_are_bit_identical(gpu_device):
    from openglue_amd.optim import Adam
    init = [t for _, t in ref.parameter_set("C2", seed=1)]
    grads = [[g.to(gpu_device) for g in gs] for gs in _grads(init, 4, seed=3)]
    runs = []
    for _ in range(2):
        params = [torch.nn.Parameter(t.to(gpu_device)) for t in init]
        opt = Adam(params, lr=1e-3, max_grad_norm=MAX_NORM, scheduler_gamma=0.97)
        norms = []
        for gs in grads:
            _set_grads(params, gs)
            opt.step()
            norms.append(opt.grad_norm.clone())
        st = opt.state_dict()["state"]
        runs.append(([p.detach().clone() for p in params], [st[i]["exp_avg"] for i in range(len(params))],
                     [st[i]["exp_avg_sq"] for i in range(len(params))], norms))
    for a, b in zip(runs[0], runs[1]):
        assert all(torch.equal(x, y) for x, y in zip(a, b))
    assert all(bool(torch.isfinite(n)) and float(n) > 0 for n in runs[0][3])


def _small_model(dev):
    from openglue_amd.superglue import SuperGlue
    cfg = syn.make_config(descriptor_dim=64, num_stages=2, num_heads=4, num_iters=20)
    model = SuperGlue(cfg)
    model.load_state_dict(syn.make_state_dict(cfg, seed=0))
    return cfg, model.to(dev)


def test_contract_after_a_step(gpu_device):
    """Gradients zeroed in place and still the same memory, a second backward accumulates there, every parameter's version counter
    moved, and the module in eval() serves the UPDATED weights: bit-identical to a fresh module loaded from its state_dict()."""
    from examples.train_loop import make_pairs, nll
    from openglue_amd.optim import Adam
    from openglue_amd.superglue import SuperGlue
    cfg, model = _small_model(gpu_device)
    data, gt0, gt1 = make_pairs(2, 128, 64, gpu_device)
    with torch.no_grad():
        before = model.eval()(data)["scores"].clone()          # packs (and caches) the weights as they are now
    model.train()
    opt = Adam(model.parameters(), lr=1e-3, max_grad_norm=MAX_NORM, scheduler_gamma=0.999994)
    params = list(model.parameters())
    assert set(opt.param_groups[0]) == set(torch.optim.Adam([torch.zeros(1)]).param_groups[0])     # torch's keys, nothing else
    ptrs = [p.grad.data_ptr() for p in params]
    assert all(p.grad is not None and bool((p.grad == 0).all()) for p in params)
    nll(model(data)["scores"], gt0, gt1).backward()
    assert [p.grad.data_ptr() for p in params] == ptrs         # backward accumulated in place
    with_grad = [bool((p.grad != 0).any()) for p in params]
    assert sum(with_grad) > len(params) // 2
    old = [p.detach().clone() for p in params]
    versions = [p._version for p in params]
    opt.step()
    assert all(bool((p.grad == 0).all()) for p in params) and [p.grad.data_ptr() for p in params] == ptrs
    assert all(p._version > v for p, v in zip(params, versions))
    assert all(bool((p != o).any()) == w for p, o, w in zip(params, old, with_grad))       # a parameter without gradient and state stays
    opt.zero_grad()
    assert [p.grad.data_ptr() for p in params] == ptrs
    nll(model(data)["scores"], gt0, gt1).backward()
    assert [p.grad.data_ptr() for p in params] == ptrs and sum(bool((p.grad != 0).any()) for p in params) > len(params) // 2
    opt.zero_grad()                                             # gradients of a step that is skipped are cleared
    assert all(bool((p.grad == 0).all()) for p in params)
    with torch.no_grad():
        after = model.eval()(data)["scores"]
        fresh = SuperGlue(cfg)
        fresh.load_state_dict(model.state_dict())
        want = fresh.to(gpu_device).eval()(data)["scores"]
    assert torch.equal(after, want)
    assert not torch.equal(after, before)


def test_only_the_three_kernels_run(gpu_device):
    from openglue_amd.optim import Adam
    init = [t for _, t in ref.parameter_set("C1", seed=0)]
    grads = _grads(init, 2, seed=5)
    for max_norm, want in ((MAX_NORM, ["adam_gradnorm_kernel", "adam_prepare_kernel", "adam_update_kernel"]),
                           (None, ["adam_prepare_kernel", "adam_update_kernel"])):
        params = [torch.nn.Parameter(t.to(gpu_device)) for t in init]
        opt = Adam(params, lr=1e-3, max_grad_norm=max_norm)
        for gs in grads:                                        # the second step too: nothing is built lazily
            _set_grads(params, gs)
            names = kernel_trace.launched_kernels(opt.step)
            assert names == want, names
        if max_norm is None:
            assert math.isnan(float(opt.grad_norm))


def test_unclipped_step_equals_torch_without_clipping(gpu_device):
    """max_grad_norm=None: plain Adam.  Also the zero-gradient rule: a step on zero gradients still decays the moments and moves the
    parameters, as torch does after zero_grad(set_to_none=False)."""
    from openglue_amd.optim import Adam
    init = [t for _, t in ref.parameter_set("C1", seed=2)]
    grads = _grads(init, 6, seed=9)
    grads[3] = [torch.zeros_like(g) for g in grads[3]]
    params = [torch.nn.Parameter(t.to(gpu_device)) for t in init]
    opt = Adam(params, lr=1e-3)
    tparams = [torch.nn.Parameter(t.clone()) for t in init]
    topt = torch.optim.Adam(tparams, lr=1e-3)
    exact = ref.RefAdam([t.double() for t in init], lr=1e-3)
    for s, gs in enumerate(grads):
        _set_grads(params, gs)
        before = params[0].detach().clone()
        opt.step()
        if s == 3:
            assert bool((params[0] != before).any())
        for p, g in zip(tparams, gs):
            p.grad = g.clone()
        topt.step()
        exact.step(gs)
    _assert_within_bar("C1 x 6 steps, no clipping, one zero gradient", _our_errors(exact, params, opt), _torch_errors(exact, tparams, topt))


def test_checkpoints_travel_both_ways(gpu_device):
    """k steps under torch.optim.Adam on the GPU -> state_dict() -> this class -> j steps, and the reverse; the continued run must be
    as close to float64 as torch's own uninterrupted fp32 run (the parity bar)."""
    from openglue_amd.optim import Adam
    k, j, lr = 6, 6, 1e-3
    init = [t for _, t in ref.parameter_set("C1", seed=3)]
    grads = _grads(init, k + j, seed=13)
    exact, tparams, topt, _, clipped = _torch_cpu_and_ref(init, grads, lr, 1.0)
    assert 0 < clipped < k + j
    torchs = _torch_errors(exact, tparams, topt)
    fresh = lambda: [torch.nn.Parameter(t.to(gpu_device)) for t in init]

    def torch_steps(params, opt, gss):
        for gs in gss:
            _set_grads(params, gs)
            torch.nn.utils.clip_grad_norm_(params, MAX_NORM)
            opt.step()
            opt.zero_grad(set_to_none=False)

    def our_steps(params, opt, gss):
        for gs in gss:
            _set_grads(params, gs)
            opt.step()

    # torch -> ours
    pa = fresh()
    oa = torch.optim.Adam(pa, lr=lr)
    torch_steps(pa, oa, grads[:k])
    pb = [torch.nn.Parameter(p.detach().clone()) for p in pa]
    ob = Adam(pb, lr=0.5, max_grad_norm=MAX_NORM)              # lr comes from the checkpoint
    ob.load_state_dict(oa.state_dict())
    assert ob.param_groups[0]["lr"] == lr
    our_steps(pb, ob, grads[k:])
    _assert_within_bar(f"checkpoint torch x {k} -> ours x {j}", _our_errors(exact, pb, ob), torchs)
    sd = ob.state_dict()
    assert float(sd["state"][0]["step"]) == k + j and sd["state"][0]["exp_avg"].shape == pb[0].shape
    assert set(sd["param_groups"][0]) == set(oa.state_dict()["param_groups"][0])
    # ours -> torch
    pc = fresh()
    oc = Adam(pc, lr=lr, max_grad_norm=MAX_NORM)
    our_steps(pc, oc, grads[:k])
    pd = [torch.nn.Parameter(p.detach().clone()) for p in pc]
    od = torch.optim.Adam(pd, lr=0.5)
    od.load_state_dict(oc.state_dict())
    torch_steps(pd, od, grads[k:])
    _assert_within_bar(f"checkpoint ours x {k} -> torch x {j}", _torch_errors(exact, pd, od), torchs)
    # ours -> ours, through a checkpoint taken before the first step (no state yet) and after
    pe = fresh()
    oe = Adam(pe, lr=0.5, max_grad_norm=MAX_NORM)
    oe.load_state_dict(Adam(fresh(), lr=lr, max_grad_norm=MAX_NORM).state_dict())
    our_steps(pe, oe, grads[:k])
    assert all(torch.equal(a, b) for a, b in zip(pe, pc))


def test_host_steplr_equals_the_builtin_schedule(gpu_device):
    from openglue_amd.optim import Adam
    lr, gamma, steps = 1e-3, 0.9, 12
    init = [t for _, t in ref.parameter_set("C1", seed=4)]
    grads = _grads(init, steps, seed=17)
    exact, tparams, topt, _, _ = _torch_cpu_and_ref(init, grads, lr, gamma)
    torchs = _torch_errors(exact, tparams, topt)
    pa = [torch.nn.Parameter(t.to(gpu_device)) for t in init]
    oa = Adam(pa, lr=lr, max_grad_norm=MAX_NORM, scheduler_gamma=gamma)
    pb = [torch.nn.Parameter(t.to(gpu_device)) for t in init]
    ob = Adam(pb, lr=lr, max_grad_norm=MAX_NORM)
    sched = torch.optim.lr_scheduler.StepLR(ob, step_size=1, gamma=gamma)
    for gs in grads:
        _set_grads(pa, gs)
        oa.step()
        _set_grads(pb, gs)
        ob.step()
        sched.step()
    assert abs(ob.param_groups[0]["lr"] - lr * gamma ** steps) < 1e-12 * lr
    _assert_within_bar("built-in scheduler_gamma", _our_errors(exact, pa, oa), torchs)
    _assert_within_bar("host StepLR on this class", _our_errors(exact, pb, ob), torchs)


def test_moved_and_dropped_tensors_are_picked_up(gpu_device):
    """A parameter whose storage was swapped (p.data = ...) is updated where it lives now; a `.grad` the caller dropped or replaced
    (model.zero_grad() sets None) is re-attached: None counts as zero, a foreign tensor is copied in."""
    from openglue_amd.optim import Adam
    g = torch.Generator().manual_seed(0)
    init = [torch.randn(5, 3, generator=g), torch.randn(7, generator=g)]
    grads = [[torch.randn(5, 3, generator=g), torch.randn(7, generator=g)] for _ in range(2)]
    pa = [torch.nn.Parameter(t.to(gpu_device)) for t in init]
    oa = Adam(pa, lr=1e-2)
    pb = [torch.nn.Parameter(t.to(gpu_device)) for t in init]
    ob = Adam(pb, lr=1e-2)
    for s, gs in enumerate(grads):
        _set_grads(pa, gs)
        oa.step()
        if s == 1:
            old = pb[0].data
            pb[0].data = old.clone()                            # new storage
            pb[0].grad = None                                   # dropped view ...
            pb[1].grad = gs[1].to(gpu_device)                   # ... and a foreign gradient
            ob.step()
            assert pb[0].data_ptr() != old.data_ptr() and pb[0].grad is not None and bool((pb[1].grad == 0).all())
        else:
            _set_grads(pb, gs)
            ob.step()
    assert torch.equal(pa[1], pb[1])
    assert not torch.equal(pa[0], pb[0])                        # its second gradient was dropped: counted as zero
    want = ref.RefAdam([t.double() for t in init], lr=1e-2)
    want.step(grads[0])
    want.step([torch.zeros(5, 3), grads[1][1]])
    assert ref.rel_err([p.detach() for p in pb], want.params) < 1e-5


def test_whole_training_loop(gpu_device):
    """examples/train_fit.py at the sizes of test_training_loop_with_adam_reduces_the_loss: supervision -> model -> criterion -> backward ->
    the fused step.  The loss falls, and the parameters after the first step agree with torch's clip + Adam on that step's gradients."""
    from examples.train_fit import run
    lr, gamma = 1e-3, 0.999994
    losses, first_grads, model, opt, after_first = run(steps=12, pairs=2, kpts=128, dim=64, stages=2, lr=lr, gamma=gamma, log=lambda *_: None)
    print("losses", " ".join(f"{v:.4f}" for v in losses))
    assert all(np.isfinite(losses)) and losses[-1] < 0.9 * losses[0], losses
    cfg = syn.make_config(descriptor_dim=64, num_stages=2, num_heads=4, num_iters=20, side_info_size=1)
    sd = syn.make_state_dict(cfg, seed=0)
    names = [k for k, _ in model.named_parameters()]
    init = [sd[k].float().reshape(first_grads[k].shape) for k in names]
    grads = [first_grads[k].cpu() for k in names]
    exact, tparams, topt, _, _ = _torch_cpu_and_ref(init, [grads], lr, gamma)
    ours = ref.rel_err([after_first[k] for k in names], exact.params)
    torchs = ref.rel_err([p.detach() for p in tparams], exact.params)
    parity_note(f"optimizer train_fit step 1: parameter error against float64 ours {ours:.3e} torch-fp32 {torchs:.3e}")
    assert torchs > 0 and ours <= BAR * torchs, (ours, torchs)
    assert float(opt.state_dict()["state"][0]["step"]) == 12
