"""Train-mode BatchNorm on the GPU (csrc/batchnorm_train.hip: og_batchnorm_train_forward / og_batchnorm_train_backward) through the raw C ABI,
and the autograd nodes of openglue_amd.train that call it (Conv1x1, ConvReluBNTrain, MLPBlockTrain, `splits`), against float64 on the CPU.
Cases, reference and bounds: tests/batchnorm_cases.py (the bounds are derived there; tests/test_batchnorm_cases_cpu.py shows that float32 on
the CPU meets every one of them).

Every operand of a raw call has its own row stride (C + 0, 4 or 8 floats, a different one per operand); the gap columns of the inputs hold
NaN, those of the outputs a sentinel that has to survive; the workspace is filled with NaN bytes before every call.
"""
import numpy as np
import pytest
import torch

from openglue_amd import _lib
from tests import batchnorm_cases as bc

IDS = [bc.case_name(c) for c in bc.CASES]
FORWARD_Q = ("y", "mean", "invstd", "running_mean", "running_var")
BACKWARD_Q = ("dz", "dweight", "dbias")
_CACHE = {}


def _case(case):
    """The case, its float64 references (with and without the ReLU mask) and its bounds: computed once, shared, never written to."""
    if case not in _CACHE:
        k = bc.make_case(*case)
        r1, r0 = bc.reference(k, 1), bc.reference(k, 0)
        _CACHE[case] = (k, r1, r0, bc.bounds(k, r1))
    return _CACHE[case]


def _pads(pad):
    """Row-stride paddings of (a / x, dy, the output): three different ones."""
    return pad, (pad + 4) % 12, (pad + 8) % 12


def _workspace(dev, rows, C):
    ws, wp = _lib.workspace(_lib.load().og_batchnorm_train_workspace_bytes(rows, C), dev)
    ws.fill_(255)                                            # all-ones bytes: NaN as float
    return ws, wp


def _forward(dev, k, *, null=(), momentum=bc.MOMENTUM, eps=bc.EPS, weight=None, bias=None, in_place=False):
    """One og_batchnorm_train_forward on the padded operands of case k -> dict of CPU tensors: y_full [rows, ldy] (gap included), y, mean,
    invstd, running_mean, running_var (None for what `null` names: passed as NULL)."""
    pa, _, py = _pads(k.pad)
    x = bc.padded(k.a, k.C + pa, float("nan")).to(dev)
    y = x if in_place else torch.full((k.rows, k.C + py), bc.SENTINEL, device=dev)
    t = dict(weight=(k.weight if weight is None else weight).to(dev), bias=(k.bias if bias is None else bias).to(dev),
             running_mean=k.running_mean.to(dev), running_var=k.running_var.to(dev),
             mean=torch.full((k.C,), bc.SENTINEL, device=dev), invstd=torch.full((k.C,), bc.SENTINEL, device=dev))
    p = {name: (None if name in null else v.data_ptr()) for name, v in t.items()}
    ws, wp = _workspace(dev, k.rows, k.C)
    _lib.call("og_batchnorm_train_forward", dev, x.data_ptr(), x.stride(0), k.rows, k.C, p["weight"], p["bias"], float(eps), float(momentum),
              p["running_mean"], p["running_var"], y.data_ptr(), y.stride(0), p["mean"], p["invstd"], wp, _lib.STREAM)
    torch.cuda.synchronize()
    out = {name: (None if name in null else t[name].cpu()) for name in ("mean", "invstd", "running_mean", "running_var")}
    out["y_full"] = y.cpu()
    out["y"] = out["y_full"][:, :k.C]
    del ws
    return out


def _backward(dev, k, mean, invstd, relu_mask, *, null=(), weight=None, in_place=False):
    """One og_batchnorm_train_backward -> dict of CPU tensors: dz_full, dz, dweight, dbias."""
    pa, pdy, pdz = _pads(k.pad)
    a = bc.padded(k.a, k.C + pa, float("nan")).to(dev)
    dy = bc.padded(k.dy, k.C + pdy, float("nan")).to(dev)
    dz = dy if in_place else torch.full((k.rows, k.C + pdz), bc.SENTINEL, device=dev)
    t = dict(weight=(k.weight if weight is None else weight).to(dev), dweight=torch.full((k.C,), bc.SENTINEL, device=dev),
             dbias=torch.full((k.C,), bc.SENTINEL, device=dev))
    p = {name: (None if name in null else v.data_ptr()) for name, v in t.items()}
    m, s = mean.to(dev), invstd.to(dev)
    ws, wp = _workspace(dev, k.rows, k.C)
    _lib.call("og_batchnorm_train_backward", dev, a.data_ptr(), a.stride(0), dy.data_ptr(), dy.stride(0), k.rows, k.C, p["weight"], m.data_ptr(),
              s.data_ptr(), int(relu_mask), dz.data_ptr(), dz.stride(0), p["dweight"], p["dbias"], wp, _lib.STREAM)
    torch.cuda.synchronize()
    out = {name: (None if name in null else t[name].cpu()) for name in ("dweight", "dbias")}
    out["dz_full"] = dz.cpu()
    out["dz"] = out["dz_full"][:, :k.C]
    del ws
    return out


def _same(a, b):
    """Bit-equal, NaN gaps included."""
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _check(tag, got, ref, bnd, names):
    worst = {q: bc.ratio(got[q], ref[q], bnd[q]) for q in names}
    print(f"[batchnorm {tag}] error / bound: " + " ".join(f"{q} {v:.3f}" for q, v in worst.items()))
    assert all(v <= 1.0 for v in worst.values()), (tag, worst)
    return worst


@pytest.mark.gpu
@pytest.mark.parametrize("case", bc.CASES, ids=IDS)
def test_forward_against_float64(gpu_device, case):
    """y, save_mean, save_invstd and both running statistics of every case against float64 (running_var: the unbiased variance, the biased
    one at one row); the gap columns of y; y aliasing x; every optional pointer NULL on its own; momentum 0 and 1; two runs.
    Worst error / bound over the nine cases, measured on an MI355X: y 0.17, mean 0.03, invstd 0.09, running_mean 0.008,
    running_var 0.007 (float32 on the CPU: 0.51, 0.06, < 0.005, 0.02, 0.01)."""
    dev = gpu_device
    k, r64, _, bnd = _case(case)
    full = _forward(dev, k)
    _check(bc.case_name(case) + " forward", full, r64, bnd, FORWARD_Q)
    _, _, py = _pads(k.pad)
    if py:
        assert bool((full["y_full"][:, k.C:] == bc.SENTINEL).all())
    again = _forward(dev, k)
    assert all(_same(again[q], full[q]) for q in ("y_full",) + FORWARD_Q[1:])                                # no atomics
    alias = _forward(dev, k, in_place=True)
    assert _same(alias["y"], full["y"]) and all(_same(alias[q], full[q]) for q in FORWARD_Q[1:])
    if k.pad:
        assert bool(torch.isnan(alias["y_full"][:, k.C:]).all())                                             # the gap of x is not written
    ones, zeros = torch.ones(k.C), torch.zeros(k.C)
    expect = {"weight": _forward(dev, k, weight=ones), "bias": _forward(dev, k, bias=zeros)}
    ref_ones = bc.reference(k, 1, weight=ones)
    assert bc.ratio(expect["weight"]["y"], ref_ones["y"], bc.bounds(k, ref_ones, weight=ones)["y"]) <= 1.0
    for name in ("weight", "bias", "running_mean", "running_var", "mean", "invstd"):
        part = _forward(dev, k, null=(name,))
        want = expect.get(name, full)
        for q in ("y_full",) + FORWARD_Q[1:]:
            if q != name:
                assert _same(part[q], want[q]), (name, q)
    still = _forward(dev, k, momentum=0.0)
    assert _same(still["running_mean"], k.running_mean) and _same(still["running_var"], k.running_var)
    assert _same(still["y_full"], full["y_full"])
    jump = _forward(dev, k, momentum=1.0)
    assert _same(jump["running_mean"], jump["mean"]) and _same(jump["mean"], full["mean"])


@pytest.mark.gpu
@pytest.mark.parametrize("case", bc.CASES, ids=IDS)
def test_backward_against_float64(gpu_device, case):
    """dz, dweight and dbias of every case against float64 with and without the ReLU mask, on the save_mean / save_invstd of the forward
    call; exact zeros of dz where a == 0; the dead channel; dz aliasing dy; dweight, dbias and weight NULL; the gap of dz; two runs.
    Worst error / bound over the nine cases, measured on an MI355X: dz 0.10, dweight 0.07, dbias 0.03 (float32 on the CPU: 0.08, 0.14,
    0.03)."""
    dev = gpu_device
    k, r1, r0, bnd = _case(case)
    fwd = _forward(dev, k)
    _, _, pdz = _pads(k.pad)
    for relu_mask, ref in ((1, r1), (0, r0)):
        full = _backward(dev, k, fwd["mean"], fwd["invstd"], relu_mask)
        _check(f"{bc.case_name(case)} backward mask {relu_mask}", full, ref, bnd, BACKWARD_Q)
        if pdz:
            assert bool((full["dz_full"][:, k.C:] == bc.SENTINEL).all())
        if relu_mask:
            assert bool((full["dz"][k.a == 0] == 0).all())                       # exactly 0, the tie z == 0 of the sparse channel included
            assert bool((full["dz"][k.a > 0] != 0).any()) or k.rows < 31
        else:
            assert bool((full["dz"][k.a == 0] != 0).any()) or k.rows == 1
        if k.C >= 8:
            assert bool((full["dweight"][bc.DEAD] == 0).all())
            assert bool((full["dz"][:, bc.DEAD] == 0).all()) == bool(relu_mask)
        again = _backward(dev, k, fwd["mean"], fwd["invstd"], relu_mask)
        assert all(_same(again[q], full[q]) for q in ("dz_full", "dweight", "dbias"))
        alias = _backward(dev, k, fwd["mean"], fwd["invstd"], relu_mask, in_place=True)
        assert _same(alias["dz"], full["dz"]) and _same(alias["dweight"], full["dweight"]) and _same(alias["dbias"], full["dbias"])
        for name in ("dweight", "dbias"):
            part = _backward(dev, k, fwd["mean"], fwd["invstd"], relu_mask, null=(name,))
            assert _same(part["dz_full"], full["dz_full"])
            other = "dbias" if name == "dweight" else "dweight"
            assert _same(part[other], full[other])
    ones = torch.ones(k.C)
    unit = _backward(dev, k, fwd["mean"], fwd["invstd"], 1, weight=ones)
    none = _backward(dev, k, fwd["mean"], fwd["invstd"], 1, null=("weight",))
    assert all(_same(none[q], unit[q]) for q in ("dz_full", "dweight", "dbias"))


@pytest.mark.gpu
def test_refusals_and_workspace_size(gpu_device):
    """Channel counts 6 and 0, a row stride below the channel count or not a multiple of 4, a pointer 4 bytes off, eps = 0, momentum = 1.5,
    rows = 0: the error code, and nothing written.  og_batchnorm_train_workspace_bytes is (nblk C 2 + 3 C) 4 bytes and 0 for these."""
    lib = _lib.load()
    dev = gpu_device
    INVALID, SHAPE, ALIGN = -1, -2, -3
    for rows, C, _, _ in bc.CASES + [bc.ROW0_SHAPE + (0, 0)]:
        nblk = (rows + bc.ROWS_PER_BLOCK - 1) // bc.ROWS_PER_BLOCK
        assert lib.og_batchnorm_train_workspace_bytes(rows, C) == (nblk * C * 2 + 3 * C) * 4
    for rows, C in ((8, 6), (8, 0), (0, 8), (8, 2), (-1, 8)):
        assert lib.og_batchnorm_train_workspace_bytes(rows, C) == 0
    rows, C, ld = 8, 8, 16
    S = bc.SENTINEL
    x = torch.randn(rows + 1, ld, device=dev)
    dy = torch.randn(rows + 1, ld, device=dev)
    outs = {n: torch.full((rows + 1, ld) if n in ("y", "dz") else (ld,), S, device=dev) for n in ("y", "dz", "mean", "invstd", "dweight", "dbias")}
    w, b = torch.ones(ld, device=dev), torch.zeros(ld, device=dev)
    rm, rv = torch.full((ld,), 0.25, device=dev), torch.full((ld,), 1.5, device=dev)
    sm, si = torch.zeros(ld, device=dev), torch.ones(ld, device=dev)
    ws, wp = _lib.workspace(lib.og_batchnorm_train_workspace_bytes(rows, ld), dev)

    def fwd(rows=rows, C=C, ldx=ld, ldy=ld, xoff=0, yoff=0, eps=1e-5, momentum=0.1):
        return lib.og_batchnorm_train_forward(x.data_ptr() + xoff, ldx, rows, C, w.data_ptr(), b.data_ptr(), eps, momentum, rm.data_ptr(),
                                              rv.data_ptr(), outs["y"].data_ptr() + yoff, ldy, outs["mean"].data_ptr(), outs["invstd"].data_ptr(), wp, None)

    def bwd(rows=rows, C=C, lda=ld, lddy=ld, lddz=ld, aoff=0, dyoff=0, dzoff=0, moff=0):
        return lib.og_batchnorm_train_backward(x.data_ptr() + aoff, lda, dy.data_ptr() + dyoff, lddy, rows, C, w.data_ptr(), sm.data_ptr() + moff,
                                               si.data_ptr(), 1, outs["dz"].data_ptr() + dzoff, lddz, outs["dweight"].data_ptr(),
                                               outs["dbias"].data_ptr(), wp, None)

    with torch.cuda.device(dev):
        assert fwd(C=6) == SHAPE and bwd(C=6) == SHAPE
        assert fwd(C=0) == INVALID and bwd(C=0) == INVALID
        assert fwd(rows=0) == INVALID and bwd(rows=0) == INVALID
        assert fwd(ldx=4) == SHAPE and fwd(ldy=4) == SHAPE                      # ld < channels
        assert bwd(lda=4) == SHAPE and bwd(lddy=4) == SHAPE and bwd(lddz=4) == SHAPE
        assert fwd(ldx=10) == SHAPE and fwd(ldy=14) == SHAPE                    # ld % 4 != 0
        assert bwd(lda=10) == SHAPE and bwd(lddy=14) == SHAPE and bwd(lddz=9) == SHAPE
        assert fwd(xoff=4) == ALIGN and fwd(yoff=4) == ALIGN
        assert bwd(aoff=4) == ALIGN and bwd(dyoff=4) == ALIGN and bwd(dzoff=4) == ALIGN and bwd(moff=4) == ALIGN
        assert fwd(eps=0.0) == INVALID and fwd(eps=-1e-5) == INVALID
        assert fwd(momentum=1.5) == INVALID and fwd(momentum=-0.1) == INVALID
        torch.cuda.synchronize()
        assert all(bool((t == S).all()) for t in outs.values())
        assert bool((rm == 0.25).all()) and bool((rv == 1.5).all())
        assert fwd() == 0 and bwd() == 0                                        # the same buffers are fine when the arguments are
        torch.cuda.synchronize()
        assert bool((outs["y"][:rows, :C] != S).all()) and bool((outs["y"][:, C:] == S).all()) and bool((outs["y"][rows:] == S).all())
        assert bool((outs["dz"][:rows, :C] != S).all()) and bool((outs["dz"][:, C:] == S).all()) and bool((outs["dz"][rows:] == S).all())
    del ws


# ------------------------------------------------------------------------------------------------------------------
# the autograd nodes
def _run_nodes(dev, case, splits, cotangent="dense"):
    """feed_forward_train_autograd on the device -> dict with the keys of bc.mlp_reference (CPU tensors)."""
    from openglue_amd.train import feed_forward_train_autograd
    T, _, sizes, seed = case
    x, params, buffers, R = bc.make_mlp_case(T, None, sizes, seed)
    xd = x.to(dev).requires_grad_(True)
    p = {k: v.to(dev).requires_grad_(True) for k, v in params.items()}
    buf = {k: v.to(dev).clone() for k, v in buffers.items()}
    y = feed_forward_train_autograd(xd, p, buf, splits=splits)
    if cotangent == "dense":
        y.backward(R.to(dev))
    else:                                                    # a column slice of a wider tensor: row stride > channels
        wide = torch.full((T, sizes[-1] + 8), float("nan"), device=dev)
        wide[:, 4:4 + sizes[-1]] = R.to(dev)
        g = wide[:, 4:4 + sizes[-1]]
        assert not g.is_contiguous()
        y.backward(g)
    out = {"y": y.detach().cpu(), "grad_x": xd.grad.cpu()}
    out.update({"grad_" + k: v.grad.cpu() for k, v in p.items()})
    out.update({k: v.cpu() for k, v in buf.items()})
    return out


def _check_nodes(tag, got, ref, T, sizes):
    worst = 0.0
    for k, want in ref.items():
        if k == "min_preact":
            continue
        bound = bc.MEAN_BAR if "running" in k else bc.mlp_bound(want, T, sizes, k == "y")
        r = float((got[k].double().reshape(want.shape) - want).abs().max()) / bound
        worst = max(worst, r)
        assert r <= 1.0, (tag, k, r)
    print(f"[batchnorm nodes {tag}] worst error / bound {worst:.3f}")


@pytest.mark.gpu
@pytest.mark.parametrize("case", bc.MLP_CASES, ids=[bc.mlp_name(c) for c in bc.MLP_CASES])
def test_autograd_nodes_against_float64(gpu_device, case):
    """Conv1x1, ConvReluBNTrain and MLPBlockTrain through feed_forward_train_autograd: the output, every gradient (dx, conv weights and
    biases, dgamma, dbeta) and the running statistics after the call (one update per row range, in order) against float64 autograd with
    BatchNorm applied per row range; with a dense and with a non-contiguous upstream gradient.  Worst error / bound on an MI355X: 0.02."""
    T, splits, sizes, seed = case
    x, params, buffers, R = bc.make_mlp_case(*case)
    ref = bc.mlp_reference(x, params, buffers, R, splits)
    assert ref["min_preact"] > bc.MLP_MIN_PREACT
    for cotangent in ("dense", "slice"):
        got = _run_nodes(gpu_device, case, splits, cotangent)
        _check_nodes(f"{bc.mlp_name(case)} {cotangent}", got, ref, T, sizes)


@pytest.mark.gpu
def test_row_ranges_are_honoured(gpu_device):
    """splits = (37, 91), (91, 37) and None on the same input: three different results, each the float64 one of its own ranges (two
    sequential running-statistics updates are not one update over all rows); row ranges that do not add up to the rows raise."""
    from openglue_amd.train import feed_forward_train_autograd
    case = bc.MLP_CASES[0]
    T, _, sizes, seed = case
    x, params, buffers, R = bc.make_mlp_case(T, None, sizes, seed)
    runs, refs = [], []
    for splits in ((37, 91), (91, 37), None):
        refs.append(bc.mlp_reference(x, params, buffers, R, splits))
        runs.append(_run_nodes(gpu_device, case, splits))
        _check_nodes(f"splits {splits}", runs[-1], refs[-1], T, sizes)
    for i in range(3):
        for j in range(i + 1, 3):
            for k in ("y", "grad_x", "grad_2.weight", "2.running_mean", "2.running_var"):
                bound = bc.MEAN_BAR if "running" in k else bc.mlp_bound(refs[i][k], T, sizes, k == "y")
                assert float((runs[j][k].double() - refs[i][k]).abs().max()) > 20 * bound, (i, j, k)
    xd = x.to(gpu_device)
    for chain in (sizes, (36, 64, 32, 16)):                  # MLPBlockTrain, ConvReluBNTrain
        _, p, b, _ = bc.make_mlp_case(T, None, chain, seed)
        p = {k: v.to(gpu_device) for k, v in p.items()}
        b = {k: v.to(gpu_device) for k, v in b.items()}
        with pytest.raises(ValueError):
            feed_forward_train_autograd(xd, p, b, splits=(37, 90))


# ------------------------------------------------------------------------------------------------------------------
# the row-0 case
@pytest.mark.gpu
def test_statistics_do_not_hang_on_row_0(gpu_device):
    """65536 x 256; channels 0-15 sit at 10 +- 1e-3 with ROW 0 set to 0 (a ReLU zero), channels 16-31 the same with a typical row 0, the
    rest Gaussian.  Bars: save_invstd 1e-4 relative to 1 / sqrt(var64 + eps), mean 1e-5 (those of
    test_batchnorm_train_large_and_offset_channels).

    With a channel-wide shift by row 0 (the scheme pass 1 had) channels 0-15 ran unshifted.  Predicted by the numpy restatement
    (tests/batchnorm_cases.py, emulate_stats_row0_shift): 5.7e-4 on channels 0-15, 4.9e-8 on 16-31.  Measured on an MI355X with that
    kernel: channels 0-15 5.72e-04, channels 16-31 6.46e-08, Gaussian 5.94e-08, mean error 4.5e-07 -- the bar was missed as predicted.
    With per-lane pivots and Chan's merge (emulation: 7.3e-7 / 4.0e-7 / 6.0e-8): measured channels 0-15 7.32e-07, channels 16-31
    4.02e-07, Gaussian 6.22e-08, mean error 4.5e-07."""
    from openglue_amd.train import batch_norm_train
    x = bc.row0_case()
    T, C = x.shape
    rm, rv = torch.zeros(C, device=gpu_device), torch.ones(C, device=gpu_device)
    _, mean, invstd = batch_norm_train(x.to(gpu_device), None, None, rm, rv, bc.MOMENTUM, bc.EPS, return_stats=True)
    m64, _, _ = bc.stats64(x)
    err = bc.invstd_error(invstd.cpu().numpy(), x)
    merr = np.abs(mean.cpu().double().numpy() - m64)
    print(f"[batchnorm row 0] relative invstd error: channels 0-15 {err[:16].max():.2e}, channels 16-31 {err[16:32].max():.2e}, "
          f"Gaussian {err[32:].max():.2e}; mean error {merr[:16].max():.2e} / {merr[16:32].max():.2e} / {merr[32:].max():.2e}")
    assert merr.max() < bc.MEAN_BAR
    assert err.max() < bc.INVSTD_BAR
