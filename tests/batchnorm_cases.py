"""Seeded inputs, the float64 reference and the bounds for the tests of the train-mode BatchNorm kernels (csrc/batchnorm_train.hip:
og_batchnorm_train_forward / og_batchnorm_train_backward) and of the autograd nodes of openglue_amd.train that call them.  Plain torch
and numpy on the CPU; tests/test_batchnorm_cases_cpu.py and tests/test_gpu_batchnorm_train.py both build their inputs here.

A case is (rows, C, row-stride padding, seed) -> a pre-activation z, a = relu(z), weight, bias, running statistics that are not 0 / 1 and
a dense cotangent dy.  Every case with C >= 8 carries four special channels at fixed indices (DEAD, CONST, OFFSET, SPARSE); the others
are Gaussian with both signs in every channel.

Bounds (all scales from the float64 reference, none from the output under test).  u_c = 2^-22 max_t|a[t, c]| invstd64_c is what xhat
cannot know better because a and mean are float32 values: negligible on ordinary channels, ~2e-4 on the offset channel.
  mean, running_mean   1e-5 absolute                       the bars of test_batchnorm_train_large_and_offset_channels
  invstd               1e-4 relative to 1 / sqrt(var64 + eps)
  running_var          1e-5 absolute
  y                    2e-5 max(1, max|y64_c|) + |w_c| u_c
  dbias                2e-6 sum_t|dy|                      L1 scales: aware of cancellation; 2e-6 is the bar of og_colsum_f32's test
  dweight              2e-6 sum_t|dy xhat64| + u_c sum_t|dy|
  dz                   |w_c| invstd64_c (2e-6 S_c + u_c (|dweight64_c| / T + max_t|xhat64| sum_t|dy| / T)),
                       S_c = max_t|dy| + |dbias64_c| / T + max_t|xhat64| |dweight64_c| / T: the size of the TERMS of dz, not of dz (at 2
                       or 3 rows dz is a near-total cancellation and float32 autograd itself is ~8e-4 max|dz| off)
The forms are derived, not measured; test_float32_cpu_attains_every_bound keeps them attainable.

`emulate_*` restate the arithmetic of the forward's statistics passes in numpy (float32 where the kernel is float32, in its order).
"""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np
import torch

from oracle import superglue_oracle as orc

MOMENTUM, EPS = 0.1, 1e-5
ROWS_PER_BLOCK = 32                                # BN_ROWS_PER_BLOCK of csrc/batchnorm_train.hip
DEAD, CONST, OFFSET, SPARSE = 1, 2, 4, 7           # channel indices of the special channels (C >= 8)
CONST_VALUE = 3.7
SENTINEL = -7.25                                   # what the gap columns of an output hold before the call, and after

# (rows, C, pad, seed): the smallest shapes that hit each edge
CASES = [
    (1, 4, 4, 0),          # a single row, a single lane
    (2, 4, 8, 0),          # fewer rows than waves
    (3, 8, 0, 0),          # fewer rows than waves
    (31, 36, 4, 0),        # one slab, one row short
    (32, 64, 8, 0),        # exactly one slab
    (33, 260, 4, 0),       # slab edge + 1, second channel block with a 4-channel tail
    (150, 512, 0, 0),      # two full channel blocks, 5 slabs
    (1000, 132, 8, 0),     # 32 slabs, ragged last
    (4099, 256, 4, 0),     # 129 slabs, ragged over the four folding waves
]
ROW0_SHAPE = (65536, 256)
MEAN_BAR, INVSTD_BAR, RUNNING_VAR_BAR = 1e-5, 1e-4, 1e-5


def case_name(case) -> str:
    return "r%d_c%d_pad%d" % tuple(case[:3])


def special_channels(C):
    return (DEAD, CONST, OFFSET, SPARSE) if C >= 8 else ()


def ordinary_channels(C):
    return [c for c in range(C) if c not in special_channels(C)]


def make_case(rows, C, pad, seed):
    """-> namespace(rows, C, pad, z, a, weight, bias, running_mean, running_var, dy): float32 CPU tensors, z / a / dy [rows, C]."""
    g = torch.Generator().manual_seed(1000003 * seed + 131 * rows + C)
    z = torch.randn(rows, C, generator=g)
    cols = torch.arange(C)
    if rows >= 2:                                  # both an active and an inactive entry in every channel
        z[cols % rows, cols] = z[cols % rows, cols].abs()
        z[(cols + 1) % rows, cols] = -z[(cols + 1) % rows, cols].abs()
    else:
        z[0] = z[0].abs() * (1.0 - 2.0 * (cols % 2))
    z = torch.where((z > 0) & (z < 1e-3), z + 1e-3, z)        # the ReLU mask is never a rounding question
    if C >= 8:
        z[:, DEAD] = -torch.randn(rows, generator=g).abs() - 0.1
        z[:, CONST] = CONST_VALUE
        z[:, OFFSET] = 10.0 + 1e-2 * torch.randn(rows, generator=g)
        keep = torch.rand(rows, generator=g) >= 0.9
        keep[0], keep[rows - 1] = False, True                  # at least one exact zero (the ReLU tie z == 0) and one value
        z[:, SPARSE] = torch.where(keep, 5.0 * torch.randn(rows, generator=g).abs() + 1e-3, torch.zeros(rows))
    sign = 1.0 - 2.0 * (torch.rand(C, generator=g) < 0.3).float()
    return SimpleNamespace(
        rows=rows, C=C, pad=pad, z=z, a=torch.relu(z),
        weight=(torch.rand(C, generator=g) + 0.5) * sign, bias=torch.randn(C, generator=g),
        running_mean=0.5 * torch.randn(C, generator=g), running_var=torch.rand(C, generator=g) + 0.5,
        dy=torch.randn(rows, C, generator=g))


def padded(t, ld, fill):
    """[rows, C] -> a [rows, ld] tensor with t in the first C columns and `fill` in the gap; the [rows, C] view of it is out[:, :C]."""
    out = torch.full((t.shape[0], ld), float(fill), dtype=t.dtype, device=t.device)
    out[:, :t.shape[1]] = t
    return out


def reference(case, relu_mask=1, momentum=MOMENTUM, eps=EPS, dtype=torch.float64, weight=None, bias=None):
    """The plain formulas of oracle.batchnorm_train in `dtype` under autograd (not F.batch_norm: it refuses one row).  The leaf is z
    (relu(z64) == a exactly), with relu_mask == 0 it is a.  -> dict of `dtype` tensors: y, mean, invstd, xhat, running_mean,
    running_var, dz, dweight, dbias for the backward pass of sum(y * dy)."""
    w = (case.weight if weight is None else weight).detach().to(dtype).clone().requires_grad_(True)
    b = (case.bias if bias is None else bias).detach().to(dtype).clone().requires_grad_(True)
    leaf = (case.z if relu_mask else case.a).detach().to(dtype).clone().requires_grad_(True)
    a = torch.relu(leaf) if relu_mask else leaf
    y, rm, rv = orc.batchnorm_train(a, w, b, case.running_mean.to(dtype), case.running_var.to(dtype), momentum, eps)
    (y * case.dy.to(dtype)).sum().backward()
    with torch.no_grad():
        mean = a.mean(dim=0)
        invstd = 1.0 / torch.sqrt(((a - mean) ** 2).mean(dim=0) + eps)
        xhat = (a - mean) * invstd
    return dict(y=y.detach(), mean=mean, invstd=invstd, xhat=xhat, running_mean=rm.detach(), running_var=rv.detach(),
                dz=leaf.grad, dweight=w.grad, dbias=b.grad)


def bounds(case, ref64, weight=None):
    """Per-channel bounds [C] (float64) of every quantity, from the float64 reference `ref64` of the same case."""
    T = case.rows
    w = (case.weight if weight is None else weight).double().abs()
    a, dy = case.a.double(), case.dy.double()
    invstd, xhat = ref64["invstd"].double(), ref64["xhat"].double()
    u = 2.0 ** -22 * a.abs().amax(0) * invstd
    l1_dy, max_dy, max_xhat = dy.abs().sum(0), dy.abs().amax(0), xhat.abs().amax(0)
    dwt, dbs = ref64["dweight"].double().abs(), ref64["dbias"].double().abs()
    S = max_dy + dbs / T + max_xhat * dwt / T
    C = case.C
    return dict(
        mean=torch.full((C,), MEAN_BAR, dtype=torch.float64), running_mean=torch.full((C,), MEAN_BAR, dtype=torch.float64),
        invstd=INVSTD_BAR * invstd, running_var=torch.full((C,), RUNNING_VAR_BAR, dtype=torch.float64),
        y=2e-5 * ref64["y"].double().abs().amax(0).clamp(min=1.0) + w * u,
        dbias=2e-6 * l1_dy,
        dweight=2e-6 * (dy * xhat).abs().sum(0) + u * l1_dy,
        dz=w * invstd * (2e-6 * S + u * (dwt / T + max_xhat * l1_dy / T)))


def ratio(got, want, bound):
    """The worst |got - want| / bound over a tensor whose last axis is the channel axis of `bound`.  A zero bound (the dweight of a dead
    channel) admits a zero error only: 0 there, inf for anything else; a NaN in `got` gives NaN, which no `<= 1` lets through."""
    err = (got.detach().cpu().double() - want.double()).abs()
    r = torch.where(err == 0, torch.zeros_like(err), err / bound)
    return float("nan") if bool(torch.isnan(r).any()) else float(r.max())


def row0_case(seed=11):
    """65536 x 256: channels 0-15 are 10 + 1e-3 N(0, 1) with ROW 0 set to 0 (a ReLU zero in a channel that otherwise sits at
    10 +- 1e-3), channels 16-31 the same with a typical row 0, the rest Gaussian."""
    g = torch.Generator().manual_seed(seed)
    T, C = ROW0_SHAPE
    x = torch.randn(T, C, generator=g)
    x[:, :32] = 10.0 + 1e-3 * x[:, :32]
    x[0, :16] = 0.0
    return x


def stats64(x, eps=EPS):
    x64 = torch.as_tensor(x).double()
    mean = x64.mean(0)
    var = ((x64 - mean) ** 2).mean(0)
    return mean.numpy(), var.numpy(), (1.0 / torch.sqrt(var + eps)).numpy()


def invstd_error(invstd, x, eps=EPS):
    """|invstd - invstd64| sqrt(var64 + eps) per channel: the quantity the 1e-4 bar is about."""
    _, var, inv64 = stats64(x, eps)
    return np.abs(np.asarray(invstd, dtype=np.float64) - inv64) * np.sqrt(var + eps)


# ------------------------------------------------------------------------------------------------------------------
# the forward's statistics passes in numpy
def _slabs(x):
    """x [T, C] float32 -> [nblk, 8, 4, C] (slab, step, wave, channel): row r of a slab goes to wave r % 4; plus the valid-row mask."""
    T, C = x.shape
    nblk = (T + ROWS_PER_BLOCK - 1) // ROWS_PER_BLOCK
    full = np.zeros((nblk * ROWS_PER_BLOCK, C), dtype=np.float32)
    full[:T] = x
    valid = np.zeros(nblk * ROWS_PER_BLOCK, dtype=bool)
    valid[:T] = True
    return full.reshape(nblk, 8, 4, C), valid.reshape(nblk, 8, 4, 1), nblk


def _fma32(a, b, c):
    """fmaf on float32 arrays: the product of two float32 is exact in float64."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def _fold_waves_double(v):
    """[nblk, C] float64 terms -> [C]: wave w of the finalize kernel adds the slabs w, w + 4, ... in order, the waves meet in wave order."""
    tot = None
    for w in range(4):
        s = np.zeros(v.shape[1], dtype=np.float64)
        for i in range(w, v.shape[0], 4):
            s = s + v[i]
        tot = s if tot is None else tot + s
    return tot


def emulate_stats_row0_shift(x, eps=EPS):
    """The scheme the kernel had before the per-lane pivots: every row of a channel shifted by k = x[0][c]; per lane s1 += d,
    s2 = fma(d, d, s2) over its 8 rows in float32, the four waves added in order in float32, the slabs folded in double,
    var = s2 / n - dm^2.  -> mean, invstd (float64 arrays of float32 values)."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    eps = float(np.float32(eps))                                   # the entry point takes a float
    T = x.shape[0]
    xs, valid, nblk = _slabs(x)
    k = x[0]
    s1 = np.zeros((nblk, 4, x.shape[1]), dtype=np.float32)
    s2 = np.zeros_like(s1)
    for step in range(8):
        d = np.where(valid[:, step], xs[:, step] - k, np.float32(0)).astype(np.float32)
        s1 = (s1 + d).astype(np.float32)
        s2 = _fma32(d, d, s2)
    b1, b2 = s1[:, 0], s2[:, 0]
    for w in range(1, 4):
        b1, b2 = (b1 + s1[:, w]).astype(np.float32), (b2 + s2[:, w]).astype(np.float32)
    S1, S2 = _fold_waves_double(b1.astype(np.float64)), _fold_waves_double(b2.astype(np.float64))
    dm = S1 / T
    var = np.maximum(S2 / T - dm * dm, 0.0)
    return (k.astype(np.float64) + dm).astype(np.float32).astype(np.float64), (1.0 / np.sqrt(var + eps)).astype(np.float32).astype(np.float64)


def emulate_stats(x, eps=EPS):
    """The kernel's scheme (csrc/batchnorm_train.hip, bn_partial_kernel + bn_finalize_kernel): every lane takes the FIRST row it reads in
    its slab as its pivot and reduces its (up to) 8 rows to (mean, M2) in float32; the four waves are merged in wave order with Chan's
    pairwise formula in float32; the slabs' (mean, M2) are folded in double about the mean of slab 0 with n_i from the slab index.
    -> mean, invstd (float64 arrays of float32 values)."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    eps = float(np.float32(eps))                                   # the entry point takes a float
    T, C = x.shape
    xs, valid, nblk = _slabs(x)
    f32 = np.float32
    p = xs[:, 0]                                                   # [nblk, 4, C]: the lane's first row
    s1 = np.zeros((nblk, 4, C), dtype=f32)
    s2 = np.zeros_like(s1)
    for step in range(1, 8):
        d = np.where(valid[:, step], xs[:, step] - p, f32(0)).astype(f32)
        s1 = (s1 + d).astype(f32)
        s2 = _fma32(d, d, s2)
    nl = valid.sum(axis=1).astype(f32)                             # [nblk, 4, 1] rows of each lane
    with np.errstate(divide="ignore"):
        inv = np.where(nl > 0, f32(1) / nl, f32(0)).astype(f32)
    mean = np.where(nl > 0, (p + (s1 * inv).astype(f32)).astype(f32), f32(0)).astype(f32)
    m2 = np.where(nl > 0, np.maximum((s2 - ((s1 * s1).astype(f32) * inv).astype(f32)).astype(f32), f32(0)), f32(0)).astype(f32)
    na, ma, qa = nl[:, 0], mean[:, 0], m2[:, 0]
    for w in range(1, 4):
        nb = nl[:, w]
        n = (na + nb).astype(f32)
        f = (nb / n).astype(f32)
        d = (mean[:, w] - ma).astype(f32)
        ma_new = (ma + (d * f).astype(f32)).astype(f32)
        qa = (qa + (m2[:, w] + ((d * d).astype(f32) * (na * f).astype(f32)).astype(f32)).astype(f32)).astype(f32)
        ma, na = ma_new, n
    ni = np.full((nblk, 1), float(ROWS_PER_BLOCK))
    ni[-1, 0] = T - ROWS_PER_BLOCK * (nblk - 1)
    K = ma[0].astype(np.float64)
    d = ma.astype(np.float64) - K
    S1, S2 = _fold_waves_double(ni * d), _fold_waves_double(qa.astype(np.float64) + ni * d * d)
    dm = S1 / T
    var = np.maximum(S2 / T - dm * dm, 0.0)
    return (K + dm).astype(f32).astype(np.float64), (1.0 / np.sqrt(var + eps)).astype(f32).astype(np.float64)


# channel kinds of the emulation's table (row 0 set to 0): (centre, spread) -> relative invstd error predicted for the row-0 shift at 65536 rows
ROW0_TABLE = (((10.0, 1e-2), 1.2e-4), ((10.0, 1e-3), 5.2e-4), ((10.0, 1e-4), 7.2e-4), ((1000.0, 1.0), 1.1e-4))
ROW0_TABLE_ROWS = ((8192, 2.8e-5), (1000, 1.3e-5))                 # (10, 1e-2) at fewer rows


def table_input(centre, spread, rows=65536, channels=16, seed=3, row0_zero=True):
    g = torch.Generator().manual_seed(seed)
    x = (centre + spread * torch.randn(rows, channels, generator=g, dtype=torch.float64)).float()
    if row0_zero:
        x[0] = 0.0
    return x.numpy()


# ------------------------------------------------------------------------------------------------------------------
# the autograd nodes of openglue_amd.train (Conv1x1, ConvReluBNTrain, MLPBlockTrain through feed_forward_train_autograd)
# (T, splits, channel sizes, seed): the seed is the first whose float64 pre-activations all keep |z| > MLP_MIN_PREACT
MLP_CASES = [
    (128, (37, 91), (36, 260, 64), 0),             # MLPBlockTrain, a second channel block with a 4-channel tail, ragged row ranges
    (130, (65, 65), (64, 512, 64), 4),             # MLPBlockTrain at the width of the C2 message MLP
    (33, None, (8, 32, 64, 32), 0),                # three convs: the ConvReluBNTrain chain + Conv1x1
]
MLP_MIN_PREACT = 1e-5                              # float32 GEMM error is ~1e-6 here: no ReLU decision of the device run can differ


def mlp_name(case) -> str:
    T, splits, sizes, _ = case
    return "t%d_%s_%s" % (T, "x".join(map(str, splits)) if splits else "whole", "-".join(map(str, sizes)))


def make_mlp_case(T, splits, sizes, seed):
    """-> (x [T, sizes[0]], params {nn.Sequential name: tensor}, buffers {running statistics}, R [T, sizes[-1]] dense cotangent), float32."""
    g = torch.Generator().manual_seed(7919 * seed + 31 * T + sizes[1])
    x = torch.randn(T, sizes[0], generator=g)
    params, buffers = {}, {}
    for i, (cin, cout) in enumerate(zip(sizes[:-1], sizes[1:])):
        params[f"{3 * i}.weight"] = torch.randn(cout, cin, 1, generator=g) / cin ** 0.5
        params[f"{3 * i}.bias"] = 0.1 * torch.randn(cout, generator=g)
        if i + 2 < len(sizes):
            params[f"{3 * i + 2}.weight"] = torch.rand(cout, generator=g) + 0.5
            params[f"{3 * i + 2}.bias"] = 0.1 * torch.randn(cout, generator=g)
            buffers[f"{3 * i + 2}.running_mean"] = 0.5 * torch.randn(cout, generator=g)
            buffers[f"{3 * i + 2}.running_var"] = torch.rand(cout, generator=g) + 0.5
    return x, params, buffers, torch.randn(T, sizes[-1], generator=g)


def mlp_reference(x, params, buffers, R, splits, dtype=torch.float64, momentum=MOMENTUM, eps=EPS):
    """FeedForwardNet in training mode under autograd in `dtype`: conv -> ReLU -> oracle.batchnorm_train per row range, the running
    statistics carried from one range to the next.  -> dict: y, grad_x, grad_<parameter name>, <buffer name> (after), min_preact."""
    n_conv = len([k for k in params if k.endswith(".weight") and params[k].dim() == 3])
    xl = x.detach().to(dtype).clone().requires_grad_(True)
    p = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in params.items()}
    buf = {k: v.detach().to(dtype).clone() for k, v in buffers.items()}
    ranges = tuple(splits) if splits else (x.shape[0],)
    h, min_preact = xl, float("inf")
    for i in range(n_conv):
        h = h @ p[f"{3 * i}.weight"][:, :, 0].T + p[f"{3 * i}.bias"]
        if i + 1 < n_conv:
            min_preact = min(min_preact, float(h.detach().abs().min()))
            h = torch.relu(h)
            bn, outs, r0 = f"{3 * i + 2}", [], 0
            for rows in ranges:
                y, buf[bn + ".running_mean"], buf[bn + ".running_var"] = orc.batchnorm_train(
                    h[r0:r0 + rows], p[bn + ".weight"], p[bn + ".bias"], buf[bn + ".running_mean"], buf[bn + ".running_var"], momentum, eps)
                outs.append(y)
                r0 += rows
            h = torch.cat(outs, 0)
    (h * R.to(dtype)).sum().backward()
    out = {"y": h.detach(), "grad_x": xl.grad, "min_preact": min_preact}
    out.update({"grad_" + k: v.grad for k, v in p.items()})
    out.update({k: v.detach() for k, v in buf.items()})
    return out


def mlp_bound(ref, T, sizes, forward=False):
    """2e-5 max|ref| max(1, sqrt(K) / 8) per tensor (the form of test_gemm_kmajor_against_float64, ten times its 2e-6 for the chain of
    products behind every tensor): K is the longest contraction on the way to it -- the widest conv input for y, and for the gradients
    the token count as well (dW, db, dgamma, dbeta contract over T; dx inherits them through the BatchNorm backward).  forward: `ref` is y."""
    K = max(sizes[:-1]) if forward else max(T, *sizes)
    return 2e-5 * float(ref.abs().max()) * max(1.0, K ** 0.5 / 8)
