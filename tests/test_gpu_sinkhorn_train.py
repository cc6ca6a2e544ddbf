"""The training Sinkhorn (csrc/sinkhorn_train.hip; forward sweeps of csrc/sinkhorn.hip on real duals) per kernel instance, against the
oracle in float64 under autograd on the CPU.

og_sinkhorn_backward picks sk_bwd_iter_kernel<CH> from ceil((n + 1) / 64), og_sinkhorn_train_forward picks
sinkhorn_sweep_kernel<CPL, RG, WPR> from n: every case here names the instances it is meant to run and fails if the profiler saw others.

Tolerances (errors are max |got - want| over a tensor; every scale comes from the float64 reference, none from the output under test):
  scores     1e-4 + 2e-6 max|ref|                      the bar of test_sinkhorn_extreme_score_range (1e-4 at ordinary ranges)
  dS         scale = max|dS_ref|.  Cap 1e-3 scale (the project's gradient bar); tight: err <= max(32 err_fp32_oracle, 2e-5 scale), with
             the float32 CPU oracle's own error on the same input (32 covers __expf against expf, the summation order and the float
             atomics; 2e-5 is the float64 bar of the exact-fp32 attention backward tests)
  d dustbin  a sum of B (m + n + 1) signed terms that can cancel: scale = the L1 norm of the float64 gradient over the bin entries of the
             augmented matrix (the augmented matrix is the leaf of the reference, _reference below); same cap and tight rule
The backward uses float atomics: two runs agree to rounding only, so only the forward is ever compared bit for bit.

The two extreme rows carry the spoiled row and column of test_sinkhorn_extreme_score_range in the gradient check as well: on those inputs
the float32 oracle stays within 2.8e-5 scale of float64 (dS) and 6.0e-6 (d dustbin), below the tenth of the cap that would have
called for the plain input.
"""
import math

import pytest
import torch

from openglue_amd import _lib
from openglue_amd.kernel_trace import launched_kernels
from oracle import superglue_oracle as orc


def _reference(S, z, iters, reg, loss_fn, dtype):
    """orc.matching_log_probs restated with the AUGMENTED matrix as the autograd leaf -> scores, dS, d dustbin, L1 norm of the bin gradient."""
    B, m, n = S.shape
    S_aug = torch.empty(B, m + 1, n + 1, dtype=dtype)
    S_aug[:, :m, :n] = S.to(dtype)
    S_aug[:, m, :] = z
    S_aug[:, :, n] = z
    S_aug.requires_grad_(True)
    norm = -math.log(m + n)
    log_a = torch.full((B, m + 1), norm, dtype=dtype)
    log_b = torch.full((B, n + 1), norm, dtype=dtype)
    log_a[:, -1] += math.log(n)
    log_b[:, -1] += math.log(m)
    scores = orc.log_sinkhorn(log_a, log_b, S_aug, iters, reg) - norm
    loss_fn(scores).backward()
    g = S_aug.grad
    bins = torch.cat([g[:, m, :].reshape(-1), g[:, :m, n].reshape(-1)])
    return scores.detach(), g[:, :m, :n].clone(), bins.sum().item(), bins.double().abs().sum().item()


def test_reference_restatement_is_the_oracle():
    """The augmented-leaf restatement computes exactly orc.matching_log_probs, scores and gradients."""
    g = torch.Generator().manual_seed(5)
    S0 = torch.randn(2, 9, 14, generator=g, dtype=torch.float64) * 3
    R = torch.randn(2, 10, 15, generator=g, dtype=torch.float64)
    sc, dS, dz, _ = _reference(S0, 0.7, 4, 0.8, lambda s: (s * R).sum(), torch.float64)
    S = S0.clone().requires_grad_(True); z = torch.tensor(0.7, dtype=torch.float64, requires_grad=True)
    want = orc.matching_log_probs(S, z, 4, 0.8)
    (want * R).sum().backward()
    assert torch.equal(sc, want.detach()) and torch.equal(dS, S.grad)
    assert abs(dz - z.grad.item()) <= 1e-12 * max(1.0, abs(dz))


def _inputs(B, m, n, scale, spoil):
    g = torch.Generator().manual_seed(B * 1000003 + m * 4099 + n * 17 + int(scale * 10))
    S = torch.randn(B, m, n, generator=g) * scale
    if spoil:                                       # test_sinkhorn_extreme_score_range: a row nobody wants and a column everybody wants
        S[0, 5, :] = -4.0 * scale
        S[-1, :, 7] = 4.0 * scale
    R = torch.randn(B, m + 1, n + 1, generator=g)
    k = max(1, round(0.6 * min(m, n)))
    gt0 = torch.full((B, m), -1, dtype=torch.long); gt1 = torch.full((B, n), -1, dtype=torch.long)
    for b in range(B):
        i = torch.randperm(m, generator=g)[:k]; j = torch.randperm(n, generator=g)[:k]
        gt0[b, i] = j; gt1[b, j] = i
    return S, R, gt0, gt1


def _gpu_run(dev, S, z, iters, reg, loss_fn):
    from openglue_amd.train import matching_log_probs
    Sg = S.to(dev).requires_grad_(True)
    zg = torch.tensor(z, device=dev, requires_grad=True)
    box = {}

    def run():
        box["scores"] = matching_log_probs(Sg, zg, iters, reg)
        loss_fn(box["scores"]).backward()
    names = launched_kernels(run)
    return box["scores"].detach().cpu(), Sg.grad.cpu(), zg.grad.item(), names


def _assert_instances(names, ch, fwd, iters):
    bwd = [k for k in names if k.startswith("sk_bwd_iter_kernel<")]
    sweeps = [k for k in names if k.startswith("sinkhorn_sweep_kernel<")]
    assert bwd == [f"sk_bwd_iter_kernel<{ch}>"] * iters, sorted(set(bwd))
    want = "sinkhorn_sweep_kernel<%d, %d, %d," % fwd
    assert len(sweeps) == iters and all(k.startswith(want) for k in sweeps), (want, sorted(set(sweeps)))
    assert not [k for k in names if k.startswith("sinkhorn_sweep_fast_kernel")], "training runs the max-subtracted sweep only"


def _check_gradients(tag, got_dS, got_dz, ref64, ref32):
    """A4: cap and tight bound on dS and d dustbin; prints every figure before it asserts."""
    _, dS64, dz64, l1 = ref64
    _, dS32, dz32, _ = ref32
    scale = dS64.abs().max().item()
    err = (got_dS.double() - dS64).abs().max().item()
    floor = (dS32.double() - dS64).abs().max().item()
    tight = max(32 * floor, 2e-5 * scale)
    errz, floorz = abs(got_dz - dz64), abs(dz32 - dz64)
    tightz = max(32 * floorz, 2e-5 * l1)
    print(f"[sk-train {tag}] dS err {err / scale:.2e} fp32-oracle {floor / scale:.2e} tol {tight / scale:.2e} (x max|dS| {scale:.2e}); "
          f"d dustbin err {errz / l1:.2e} fp32-oracle {floorz / l1:.2e} tol {tightz / l1:.2e} (x L1 {l1:.2e}; dz {dz64:.4e})")
    assert torch.isfinite(got_dS).all() and math.isfinite(got_dz)
    assert err <= 1e-3 * scale and errz <= 1e-3 * l1
    assert err <= tight, (err / scale, tight / scale)
    assert errz <= tightz, (errz / l1, tightz / l1)


def _check_scores(tag, got, ref):
    tol = 1e-4 + 2e-6 * ref.abs().max().item()
    err = (got.double() - ref).abs().max().item()
    print(f"[sk-train {tag}] scores err {err:.2e} tol {tol:.2e} (max |score| {ref.abs().max().item():.0f})")
    assert torch.isfinite(got).all() and err <= tol
    return err


# B, m, n, iters, reg, dustbin, input scale, backward CH, forward <CPL, RG, WPR>
TABLE = [
    (2, 37, 200, 7, 1.0, 0.7, 3.0, 4, (1, 4, 1)),
    (2, 130, 255, 6, 0.7, -0.5, 3.0, 4, (1, 4, 1)),          # <4> upper edge: n + 1 = 256
    (1, 300, 500, 10, 1.0, 1.0, 3.0, 9, (2, 4, 1)),
    (2, 77, 575, 5, 1.0, 1.0, 3.0, 9, (4, 2, 1)),            # <9> upper edge
    (1, 1030, 1087, 8, 1.0, 1.0, 3.0, 17, (4, 2, 2)),        # <17> upper edge; m + 1 beyond the 128 x 4 rows of the grid: waves stride; (m + 1) % 4 != 0
    (2, 600, 1500, 6, 0.8, 0.3, 3.0, 33, (4, 2, 2)),
    (1, 257, 2111, 4, 1.0, 1.0, 3.0, 33, (4, 2, 4)),         # <33> upper edge
    (1, 300, 4159, 3, 1.0, 1.0, 3.0, 65, (8, 1, 4)),         # the documented limit
    (1, 1, 4159, 2, 1.0, 1.0, 3.0, 65, (8, 1, 4)),           # one row
    (1, 2100, 3, 5, 1.0, 1.0, 3.0, 2, (1, 4, 1)),            # one column chunk, many strided rows
    (1, 64, 64, 1, 1.0, 1.0, 3.0, 2, (1, 4, 1)),             # iters == 1: du fresh and last at once
    (2, 96, 200, 30, 0.5, 0.7, 25.0, 4, (1, 4, 1)),          # extreme range: |Z|, |u|, |v| of several hundred
    (2, 96, 200, 30, 0.1, -30.0, 8.0, 4, (1, 4, 1)),
]


@pytest.mark.gpu
@pytest.mark.parametrize("case", TABLE, ids=lambda c: "B%d-%dx%d-it%d-reg%g-z%g-x%g" % c[:7])
def test_training_sinkhorn_instances_against_float64_autograd(gpu_device, case):
    """Forward and backward of train.matching_log_probs per kernel instance, dense and NLL loss, vs float64 autograd; the backward evaluates
    __expf(Z + u + v - lb) without a running maximum, and the extreme rows are what shows that the stored trajectory keeps those
    softmax weights <= 1 when |Z|, |u|, |v| are several hundred."""
    B, m, n, iters, reg, z, scale, ch, fwd = case
    S, R, gt0, gt1 = _inputs(B, m, n, scale, spoil=scale > 3.0)
    first = None
    for kind in ("dense", "nll"):
        cpu_loss = (lambda s: (s * R.to(s.dtype)).sum()) if kind == "dense" else (lambda s: orc.nll_criterion(s, gt0, gt1))
        Rg, g0, g1 = R.to(gpu_device), gt0.to(gpu_device), gt1.to(gpu_device)
        gpu_loss = (lambda s: (s * Rg).sum()) if kind == "dense" else (lambda s: orc.nll_criterion(s, g0, g1))
        ref64 = _reference(S, z, iters, reg, cpu_loss, torch.float64)
        ref32 = _reference(S, z, iters, reg, cpu_loss, torch.float32)
        scores, dS, dz, names = _gpu_run(gpu_device, S, z, iters, reg, gpu_loss)
        tag = f"{B}x{m}x{n} it{iters} reg{reg} z{z} x{scale} {kind} bwd<{ch}> fwd<{fwd[0]},{fwd[1]},{fwd[2]}>"
        _assert_instances(names, ch, fwd, iters)
        _check_scores(tag, scores, ref64[0])
        if first is None:
            first = scores
        else:
            assert torch.equal(scores, first)                 # the forward has no atomics: the same bits on every run
        _check_gradients(tag, dS, dz, ref64, ref32)


# the other side of every instance boundary: n, backward CH, forward geometry (dense loss, 2 iterations)
EDGES = [(127, 2, (1, 4, 1)), (128, 4, (1, 4, 1)), (256, 9, (1, 4, 1)), (257, 9, (2, 4, 1)), (512, 9, (2, 4, 1)), (513, 9, (4, 2, 1)),
         (576, 17, (4, 2, 1)), (1024, 17, (4, 2, 1)), (1025, 17, (4, 2, 2)), (1088, 33, (4, 2, 2)), (2048, 33, (4, 2, 2)),
         (2049, 33, (4, 2, 4)), (2112, 65, (4, 2, 4)), (4096, 65, (4, 2, 4)), (4097, 65, (8, 1, 4))]


@pytest.mark.gpu
@pytest.mark.parametrize("n,ch,fwd", EDGES, ids=[f"n{e[0]}" for e in EDGES])
def test_training_sinkhorn_instance_boundaries(gpu_device, n, ch, fwd):
    B, m, iters, reg, z = 1, 33 + n % 7, 2, 1.0, 1.0
    S, R, _, _ = _inputs(B, m, n, 3.0, spoil=False)
    cpu_loss = lambda s: (s * R.to(s.dtype)).sum()
    Rg = R.to(gpu_device)
    ref64 = _reference(S, z, iters, reg, cpu_loss, torch.float64)
    ref32 = _reference(S, z, iters, reg, cpu_loss, torch.float32)
    scores, dS, dz, names = _gpu_run(gpu_device, S, z, iters, reg, lambda s: (s * Rg).sum())
    tag = f"edge {B}x{m}x{n} it{iters} dense bwd<{ch}> fwd<{fwd[0]},{fwd[1]},{fwd[2]}>"
    _assert_instances(names, ch, fwd, iters)
    _check_scores(tag, scores, ref64[0])
    _check_gradients(tag, dS, dz, ref64, ref32)


# ----------------------------------------------------------------------------- the raw ABI
def _r4(x):
    return (x + 3) // 4 * 4


class _Raw:
    """og_sinkhorn_train_forward / og_sinkhorn_backward on caller-owned buffers."""

    def __init__(self, dev, B, m, n, iters, reg):
        self.dev, self.B, self.m, self.n, self.iters, self.reg = dev, B, m, n, iters, reg
        self.nbytes = _lib.load().og_sinkhorn_train_workspace_bytes(B, m, n, iters)
        assert self.nbytes > 0

    def fresh_ws(self):
        return _lib.workspace(self.nbytes, self.dev)

    def pad(self, S, lds, fill):
        buf = torch.full((self.B, self.m, lds), fill, dtype=torch.float32)
        buf[:, :, :self.n] = S
        return buf.to(self.dev)

    def forward(self, Sp, z, wp, z_on_device=True):
        scores = torch.empty(self.B, self.m + 1, self.n + 1, device=self.dev)
        self.zdev = torch.tensor([z], device=self.dev, dtype=torch.float32)
        _lib.call("og_sinkhorn_train_forward", self.dev, Sp.data_ptr(), Sp.shape[2], 0.0 if z_on_device else float(z),
                  self.zdev.data_ptr() if z_on_device else None, self.B, self.m, self.n, self.iters, float(self.reg), scores.data_ptr(), wp, _lib.STREAM)
        torch.cuda.synchronize()
        return scores.cpu()

    def backward(self, Sp, z, G, wp, ldds=None, z_on_device=True, want_dz=True, sentinel=-7.25):
        ldds = self.n if ldds is None else ldds
        dS = torch.full((self.B, self.m, ldds), sentinel, device=self.dev, dtype=torch.float32)
        dz = torch.full((1,), 123.0, device=self.dev)           # the entry zeroes it itself
        _lib.call("og_sinkhorn_backward", self.dev, Sp.data_ptr(), Sp.shape[2], 0.0 if z_on_device else float(z),
                  self.zdev.data_ptr() if z_on_device else None, self.B, self.m, self.n, self.iters, float(self.reg), G.data_ptr(), wp,
                  dS.data_ptr(), ldds, dz.data_ptr() if want_dz else None, _lib.STREAM)
        torch.cuda.synchronize()
        return dS.cpu(), dz.item()


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(2, 37, 53, 5, 0.7, 0.7), (1, 70, 2501, 3, 1.0, -0.5)], ids=["narrow", "wide65"])
def test_training_sinkhorn_raw_abi(gpu_device, shape):
    """What only the C entry points reach: padded leading dimensions with non-finite gap columns, ldds > n, the host-value dustbin,
    d_dustbin == NULL, and a workspace that an earlier, larger call has used."""
    B, m, n, iters, reg, z = shape
    assert n % 4
    S, R, _, _ = _inputs(B, m, n, 3.0, spoil=False)
    ref64 = _reference(S, z, iters, reg, lambda s: (s * R.double()).sum(), torch.float64)
    ref32 = _reference(S, z, iters, reg, lambda s: (s * R).sum(), torch.float32)
    scale = ref64[1].abs().max().item()
    close = 2e-5 * scale                                   # two backward runs differ by the order of the float atomics only
    raw = _Raw(gpu_device, B, m, n, iters, reg)
    G = R.to(gpu_device).contiguous()
    lds = _r4(n) + 8
    ws, wp = raw.fresh_ws()
    # the plain call: lds = round_up(n, 4), zero padding, device dustbin
    S0 = raw.pad(S, _r4(n), 0.0)
    sc0 = raw.forward(S0, z, wp)
    dS0, dz0 = raw.backward(S0, z, G, wp)
    _check_scores(f"raw {B}x{m}x{n} plain", sc0, ref64[0])
    _check_gradients(f"raw {B}x{m}x{n} plain", dS0, dz0, ref64, ref32)
    # lds > n with NaN in the gap columns, against zeros there; ldds = lds with a sentinel in dS
    Sz, Sn = raw.pad(S, lds, 0.0), raw.pad(S, lds, float("nan"))
    sc_z = raw.forward(Sz, z, wp); dS_z, dz_z = raw.backward(Sz, z, G, wp, ldds=lds)
    sc_n = raw.forward(Sn, z, wp); dS_n, dz_n = raw.backward(Sn, z, G, wp, ldds=lds)
    assert torch.equal(sc_z, sc0) and torch.equal(sc_n, sc0)
    for dS_x, dz_x in ((dS_z, dz_z), (dS_n, dz_n)):
        assert torch.all(dS_x[:, :, n:] == -7.25)                                # the gap columns of dS are not written
        assert (dS_x[:, :, :n] - dS0).abs().max().item() <= close
        _check_gradients(f"raw {B}x{m}x{n} lds {lds}", dS_x[:, :, :n], dz_x, ref64, ref32)
    # host-value dustbin
    sc_h = raw.forward(S0, z, wp, z_on_device=False)
    dS_h, dz_h = raw.backward(S0, z, G, wp, z_on_device=False)
    assert torch.equal(sc_h, sc0)
    assert (dS_h - dS0).abs().max().item() <= close
    _check_gradients(f"raw {B}x{m}x{n} host dustbin", dS_h, dz_h, ref64, ref32)
    # d_dustbin == NULL
    raw.forward(S0, z, wp)
    dS_q, _ = raw.backward(S0, z, G, wp, want_dz=False)
    assert (dS_q - dS0).abs().max().item() <= close
    # a workspace a LARGER problem has used, then overwritten with NaN: nothing of it may be read before it is written (the backward zeroes dv
    # itself)
    big = _Raw(gpu_device, B + 1, m + 9, n + 64, iters + 2, reg)
    Sb, Rb, _, _ = _inputs(B + 1, m + 9, n + 64, 3.0, spoil=False)
    wsb, wpb = big.fresh_ws()
    Sbp = big.pad(Sb, _r4(n + 64), 0.0)
    big.forward(Sbp, z, wpb); big.backward(Sbp, z, Rb.to(gpu_device).contiguous(), wpb)
    sc_r = raw.forward(S0, z, wpb); dS_r, dz_r = raw.backward(S0, z, G, wpb)
    assert torch.equal(sc_r, sc0) and (dS_r - dS0).abs().max().item() <= close
    wsb.fill_(255)                                          # all-ones bytes: NaN as float
    sc_r = raw.forward(S0, z, wpb); dS_r, dz_r = raw.backward(S0, z, G, wpb)
    assert torch.equal(sc_r, sc0) and (dS_r - dS0).abs().max().item() <= close
    _check_gradients(f"raw {B}x{m}x{n} reused workspace", dS_r, dz_r, ref64, ref32)
    del ws, wsb


@pytest.mark.gpu
def test_training_sinkhorn_refuses_what_it_cannot_run(gpu_device):
    """n = 4160 and iters = 0 on real device buffers: OG_E_INVALID from both entries, no launch."""
    lib = _lib.load()
    assert lib.og_sinkhorn_train_workspace_bytes(1, 8, 4160, 3) == 0 and lib.og_sinkhorn_train_workspace_bytes(1, 8, 4159, 0) == 0
    S = torch.zeros(1, 8, 4160, device=gpu_device); sc = torch.zeros(1, 9, 4161, device=gpu_device); dS = torch.zeros_like(S)
    ws, wp = _lib.workspace(lib.og_sinkhorn_train_workspace_bytes(1, 8, 4159, 3), gpu_device)
    for n, iters in ((4160, 3), (4159, 0)):
        assert lib.og_sinkhorn_train_forward(S.data_ptr(), 4160, 1.0, None, 1, 8, n, iters, 1.0, sc.data_ptr(), wp, None) == -1
        assert lib.og_sinkhorn_backward(S.data_ptr(), 4160, 1.0, None, 1, 8, n, iters, 1.0, sc.data_ptr(), wp, dS.data_ptr(), 4160, None, None) == -1
    del ws
