"""The training criterion on the MI355X (openglue_amd.supervision.criterion; the second half of csrc/supervision.hip) on the seeded
cases of tests/criterion_cases.py, which take every hinge branch, cross the Gram tile edges and the 256-thread strided loops,
and include exact ties, a positive that is alone in its row / column and all-zero descriptors.  Each case is compared with the
float64 autograd of the restatement (tests/supervision_ref.py) and, where the reference can run it, with the reference's own
fp32 results (tests/golden/criterion.npz).  The bound is 1e-5 throughout: relative for each loss, relative to each gradient
tensor's maximum; the restatement evaluated in fp32 on the CPU stays within 3.3e-7.

Worst measured values on an MI355X (relative errors; the regular cases with margin 0.2 and None, upstream weights (0.7, 1.9)):
  quantity      vs float64   vs fixture
  loss          8.8e-08      1.5e-07
  metric_loss   2.2e-07      1.9e-07
  grad_scores   6.0e-08      1.1e-08
  grad_desc0    3.5e-07      4.1e-07
  grad_desc1    3.5e-07      3.1e-07
The other cases, worst of any quantity: a positive alone in its line 2.3e-07, zero descriptors 2.3e-07 (their own columns
1.1e-07), exact ties 1.8e-07.  Before the two fixes in csrc/supervision.hip that these cases asked for, metric_loss came out
as 0.2661769 / 0.3234206 / 0 where the reference has 0.4661769 / 0.5234206 / 0.4 (m = 1, n = 1, m = n = 1: each lone term
short by the margin), and as 0.2269745 against 0.2628565 with the two zero descriptors.
"""
import numpy as np
import pytest
import torch

from tests import criterion_cases as cc
from tests.test_supervision_cpu import CRIT_CASES, ZC

pytestmark = pytest.mark.gpu

BOUND = 1e-5
LOSSES = ("loss", "metric_loss")
GRADS = ("grad_scores", "grad_desc0", "grad_desc1")
EDGE = (3, 65, 63, 64)
_CACHE = {}


def cached(key, make):
    """The CPU side of a case (inputs, census, float64 reference) is computed once and shared; nothing modifies it."""
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def regular(shape):
    return cached(("case", shape), lambda: cc.regular_case(shape))


def ref64(key, case, margin, weights=(cc.W_LOSS, cc.W_METRIC)):
    return cached(("ref64", key, margin, weights), lambda: cc.reference64(case, margin, weights))


def _rel(got, want):
    return float(np.abs(got - want).max() / max(np.abs(want).max(), 1e-30))


def run_hip(dev, case, margin, weights=(cc.W_LOSS, cc.W_METRIC), grad_scores=True, grad_desc=True, dtype=torch.float32, backward="weighted"):
    """supervision.criterion on the case's inputs -> (result dict like cc.reference64's, the three input tensors)."""
    from openglue_amd import supervision
    S, A, Bd, g0, g1 = case[:5]
    S = S.to(dev, dtype).requires_grad_(grad_scores)
    a, b = (t.to(dev, dtype).requires_grad_(grad_desc) for t in (A, Bd))
    lo = supervision.criterion({"gt_matches0": g0.to(dev), "gt_matches1": g1.to(dev)},
                               {"scores": S, "context_descriptors0": a, "context_descriptors1": b}, margin=margin)
    if backward == "weighted":
        (weights[0] * lo["loss"] + weights[1] * lo["metric_loss"]).backward()
    elif backward is not None:
        lo[backward].backward()
    grad = lambda t: None if t.grad is None else t.grad.cpu().double().numpy()
    out = {"loss": lo["loss"].item(), "metric_loss": lo["metric_loss"].item(),
           "grad_scores": grad(S), "grad_desc0": grad(a), "grad_desc1": grad(b)}
    return out, (S, a, b)


def errors(got, want, margin):
    """Relative error of every quantity `want` holds (a reference dict, or the fixture's arrays under a key prefix)."""
    errs = {}
    for k in LOSSES:
        if k == "metric_loss" and margin is None:
            assert got[k] == 0.0 and float(want[k]) == 0.0
            continue
        errs[k] = abs(got[k] - float(want[k])) / abs(float(want[k]))
    for k in GRADS:
        if margin is None and k != "grad_scores":
            assert got[k] is None
            continue
        errs[k] = _rel(got[k], np.asarray(want[k], dtype=np.float64))
    return errs


def fixture(name, margin):
    key = f"{name}_{'none' if margin is None else 'margin'}"
    return {k: ZC[f"{key}_{k}"] for k in LOSSES + GRADS if f"{key}_{k}" in ZC}


def check(tag, got, margin, w64, wfix=None):
    e64 = errors(got, w64, margin)
    efix = errors(got, wfix, margin) if wfix is not None else {}
    print(f"[{tag}] loss {got['loss']:.8g} metric_loss {got['metric_loss']:.8g} (float64 {w64['loss']:.8g} {w64['metric_loss']:.8g}); "
          f"relative errors vs float64 {({k: f'{v:.2e}' for k, v in e64.items()})} vs fixture {({k: f'{v:.2e}' for k, v in efix.items()})}")
    for k, v in list(e64.items()) + list(efix.items()):
        assert v < BOUND, (tag, k, v)


# ---------------------------------------------------------------------------------------------------------- a. regular cases
@pytest.mark.parametrize("shape", list(cc.REGULAR), ids=cc.case_name)
@pytest.mark.parametrize("margin", (cc.MARGIN, None), ids=("margin", "none"))
def test_regular_cases_against_float64_and_reference(gpu_device, shape, margin):
    case = regular(shape)
    cen = cached(("census", shape), lambda: cc.census(*case[1:]))
    assert cc.regular_case_ok(shape, cen) == []                   # a precondition of the generator, not of the kernels
    name = cc.case_name(shape)
    got, _ = run_hip(gpu_device, case, margin)
    check(f"{name} margin={margin}", got, margin, ref64(name, case, margin), fixture(name, margin))


# ------------------------------------------------------------------------------------------------- b. one gradient group only
def test_backward_of_one_loss_only(gpu_device):
    case, name = regular(EDGE), cc.case_name(EDGE)
    # loss.backward() alone: the NLL does not depend on the descriptors
    got, _ = run_hip(gpu_device, case, cc.MARGIN, backward="loss")
    want = ref64(name, case, cc.MARGIN, (1.0, 0.0))
    assert _rel(got["grad_scores"], want["grad_scores"]) < BOUND
    assert all((r[k] is None or not r[k].any()) for r in (got, want) for k in ("grad_desc0", "grad_desc1"))
    # metric_loss.backward() alone: the metric loss does not depend on the scores
    got, _ = run_hip(gpu_device, case, cc.MARGIN, backward="metric_loss")
    want = ref64(name, case, cc.MARGIN, (0.0, 1.0))
    assert all((r["grad_scores"] is None or not r["grad_scores"].any()) for r in (got, want))
    for k in ("grad_desc0", "grad_desc1"):
        assert _rel(got[k], want[k]) < BOUND, k


def test_backward_for_one_input_group_only(gpu_device):
    case, name = regular(EDGE), cc.case_name(EDGE)
    want = ref64(name, case, cc.MARGIN)
    got, (S, a, b) = run_hip(gpu_device, case, cc.MARGIN, grad_scores=False)
    assert S.grad is None and got["grad_scores"] is None
    for k in ("grad_desc0", "grad_desc1"):
        assert _rel(got[k], want[k]) < BOUND, k
    got, (S, a, b) = run_hip(gpu_device, case, cc.MARGIN, grad_desc=False)
    assert a.grad is None and b.grad is None
    assert _rel(got["grad_scores"], want["grad_scores"]) < BOUND


# ------------------------------------------------------------------------------------------------------ c. wrapper conversions
def test_float64_and_non_contiguous_inputs(gpu_device):
    from openglue_amd import supervision
    shape = (2, 70, 90, 128)
    case, name = regular(shape), cc.case_name(shape)
    S, A, Bd, g0, g1 = case
    S64 = torch.empty(S.shape[0], S.shape[2], S.shape[1], device=gpu_device, dtype=torch.float64).transpose(1, 2)
    S64.copy_(S)
    S64.requires_grad_(True)
    assert not S64.is_contiguous()
    a, b = (t.to(gpu_device, torch.float64).requires_grad_(True) for t in (A, Bd))
    lo = supervision.criterion({"gt_matches0": g0.to(gpu_device), "gt_matches1": g1.to(gpu_device)},
                               {"scores": S64, "context_descriptors0": a, "context_descriptors1": b}, margin=cc.MARGIN)
    (cc.W_LOSS * lo["loss"] + cc.W_METRIC * lo["metric_loss"]).backward()
    for t in (S64, a, b):
        assert t.grad.dtype == torch.float64 and t.grad.shape == t.shape
    got = {"loss": lo["loss"].item(), "metric_loss": lo["metric_loss"].item(), "grad_scores": S64.grad.cpu().numpy(),
           "grad_desc0": a.grad.cpu().numpy(), "grad_desc1": b.grad.cpu().numpy()}
    check(f"{name} float64 inputs, scores a transposed view", got, cc.MARGIN, ref64(name, case, cc.MARGIN), fixture(name, cc.MARGIN))


# -------------------------------------------------------------------------------------------- d. the ABI's NULL grad_losses
def test_abi_null_grad_losses_means_unit_weights(gpu_device):
    from openglue_amd import _lib
    dev = gpu_device
    case, name = regular(EDGE), cc.case_name(EDGE)
    S, a, b = (t.to(dev).contiguous() for t in case[:3])
    g0, g1 = (t.to(dev).contiguous() for t in case[3:5])
    B, M, N, D = EDGE
    lib = _lib.load()
    ws, wp = _lib.workspace(lib.og_criterion_workspace_bytes(B, M, N, 1), dev)
    out = torch.empty(2, device=dev, dtype=torch.float32)
    _lib.call("og_criterion_forward", dev, S.data_ptr(), g0.data_ptr(), g1.data_ptr(), a.data_ptr(), b.data_ptr(), B, M, N, D, 1,
              cc.MARGIN, out.data_ptr(), wp, _lib.STREAM)
    res = []
    for gl in (None, torch.ones(2, device=dev, dtype=torch.float32)):
        gS, gA, gB = torch.empty_like(S), torch.empty_like(a), torch.empty_like(b)
        _lib.call("og_criterion_backward", dev, g0.data_ptr(), g1.data_ptr(), a.data_ptr(), b.data_ptr(), B, M, N, D, 1, cc.MARGIN,
                  _lib.ptr(gl), wp, gS.data_ptr(), gA.data_ptr(), gB.data_ptr(), _lib.STREAM)
        torch.cuda.synchronize()
        res.append([t.cpu().double().numpy() for t in (gS, gA, gB)])
    want = ref64(name, case, cc.MARGIN, (1.0, 1.0))
    assert abs(out[0].item() - want["loss"]) < BOUND * abs(want["loss"])
    assert abs(out[1].item() - want["metric_loss"]) < BOUND * abs(want["metric_loss"])
    assert np.array_equal(res[0][0], res[1][0])                   # grad_scores: plain stores, bit-identical
    for r in res:
        for got, k in zip(r, GRADS):
            assert _rel(got, want[k]) < BOUND, k
    for k in (1, 2):                                              # the descriptor gradients are float-atomic sums
        assert _rel(res[0][k], res[1][k]) < BOUND


# ------------------------------------------------------------------------------------------------------------ e. exact ties
@pytest.mark.parametrize("ignore_copies", (False, True), ids=("unmatched_copies", "ignored_copies"))
def test_exact_ties_go_to_the_lower_index(gpu_device, ignore_copies):
    case = cached(("tie", ignore_copies), lambda: cc.tie_case(ignore_copies))
    cached(("tie census", ignore_copies), lambda: cc.tie_case_ok(case))
    info = case[5]
    got, _ = run_hip(gpu_device, case, cc.MARGIN)
    check(f"ties {info} ignore_copies={ignore_copies}", got, cc.MARGIN, ref64(("tie", ignore_copies), case, cc.MARGIN))
    if ignore_copies:
        # without a hinge of their own the higher-index copies could only receive a negative-mining share: exactly none
        assert not got["grad_desc1"][0, :, info["hi"]].any() and not got["grad_desc0"][0, :, info["hi2"]].any()
        assert got["grad_desc1"][0, :, info["lo"]].any() and got["grad_desc0"][0, :, info["lo2"]].any()


# ----------------------------------------------------------------------------------------------------------- f. determinism
def test_losses_are_bit_identical_across_a_tile_grid(gpu_device):
    case = regular((2, 130, 200, 40))
    vals = [run_hip(gpu_device, case, cc.MARGIN, backward=None)[0] for _ in range(2)]
    assert all(np.float32(vals[0][k]).tobytes() == np.float32(vals[1][k]).tobytes() for k in LOSSES)


# ------------------------------------------------------------------------------------- g. a positive alone in its row / column
@pytest.mark.parametrize("m,n", cc.SINGLE)
def test_positive_that_is_the_only_entry_of_its_line(gpu_device, m, n):
    """The reference's masked argmin of an all-inf line is 0, so it gathers d_an == d_ap: the term is `margin`, without gradient."""
    name = f"single_m{m}_n{n}"
    case = cached(("case", name), CRIT_CASES[name])
    for margin in (cc.MARGIN, None):
        got, _ = run_hip(gpu_device, case, margin)
        check(f"{name} margin={margin}", got, margin, ref64(name, case, margin), fixture(name, margin))


# ------------------------------------------------------------------------------------------------- h. all-zero descriptors
def test_zero_descriptor_columns(gpu_device):
    """F.normalize clamps an all-zero descriptor to a^ = 0: 0.25 |a^ - b^|^2 is 0.25 against a unit vector and 0 against another
    zero, and its gradient carries the clamp's 1 / 1e-12."""
    case = cached(("zero",), cc.zero_case)
    iz, jz = case[5:]
    want = ref64(("zero",), case, cc.MARGIN)
    got, _ = run_hip(gpu_device, case, cc.MARGIN)
    print(f"[zero columns {iz} / {jz}] loss {got['loss']:.8g} metric_loss {got['metric_loss']:.8g} (float64 {want['loss']:.8g} {want['metric_loss']:.8g})")
    errs = {k: abs(got[k] - want[k]) / abs(want[k]) for k in LOSSES}
    errs["grad_scores"] = _rel(got["grad_scores"], want["grad_scores"])
    for k, z in (("grad_desc0", iz), ("grad_desc1", jz)):
        assert np.isfinite(got[k]).all() and np.isfinite(want[k]).all()
        rest = np.arange(got[k].shape[2]) != z
        errs[k] = _rel(got[k][:, :, rest], want[k][:, :, rest])
        assert np.abs(want[k][:, :, z]).max() > 1e6 * np.abs(want[k][:, :, rest]).max()       # the clamp's 1 / eps
        errs[k + " zero column"] = _rel(got[k][:, :, z], want[k][:, :, z])
    print(f"[zero columns] relative errors vs float64 {({k: f'{v:.2e}' for k, v in errs.items()})}")
    for k, v in errs.items():
        assert v < BOUND, (k, v)
