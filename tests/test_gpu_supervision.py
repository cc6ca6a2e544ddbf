"""The training supervision on the MI355X (openglue_amd.supervision, csrc/supervision.hip): labels against the float64 restatement
(tests/supervision_ref.py) on every row and against the reference's own labels (tests/golden/supervision.npz) apart from counted
near ties; criterion values and gradients against the reference's autograd and the float64 restatement; determinism; memory;
and the whole training step of examples/train_step.py."""
import numpy as np
import pytest
import torch

from tests import supervision_ref as ref
from tests.test_supervision_cpu import GT_CASES, NEG, POS, Z, gt_case
from tests.util import parity_note

pytestmark = pytest.mark.gpu


def feats(k):
    B, N, _ = k.shape
    return {"keypoints": k, "local_descriptors": torch.zeros(B, N, 4, device=k.device), "side_info": torch.zeros(B, N, 1, device=k.device)}


def hip_labels(k0, k1, tr, pos, neg, apply_thresholds=False):
    from openglue_amd import supervision
    data, y = supervision.generate_gt_matches({"transformation": tr}, feats(k0), feats(k1), pos, neg, apply_thresholds=apply_thresholds)
    torch.cuda.synchronize()
    assert set(data) >= {"keypoints0", "keypoints1", "local_descriptors0", "local_descriptors1", "side_info0", "side_info1", "transformation"}
    return y["gt_matches0"].cpu(), y["gt_matches1"].cpu()


def on(tr, dev):
    return {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in tr.items()}


@pytest.mark.parametrize("name", GT_CASES)
def test_labels_against_restatement_and_reference(gpu_device, name):
    k0, k1, tr, want0, want1 = gt_case(name)
    for apply in (False, True):
        g0, g1 = hip_labels(k0.to(gpu_device), k1.to(gpu_device), on(tr, gpu_device), POS, NEG, apply)
        r0, r1 = ref.gt_matches(k0, k1, tr, POS, NEG, apply_thresholds=apply)
        assert torch.equal(g0, r0) and torch.equal(g1, r1), (apply, int((g0 != r0).sum()), int((g1 != r1).sum()))
    # default mode against the reference's own labels: only near-tie rows may differ
    g0, g1 = hip_labels(k0.to(gpu_device), k1.to(gpu_device), on(tr, gpu_device), POS, NEG)
    _, _, det = ref.gt_matches(k0, k1, tr, POS, NEG, with_details=True)
    ex0, ex1 = ref.near_tie_rows(k0, k1, det)
    d0, d1 = g0 != want0, g1 != want1
    parity_note(f"supervision labels {name} (HIP vs reference fixture): exempt={int(ex0.sum() + ex1.sum())} differ={int(d0.sum() + d1.sum())}")
    assert int((d0 & ~ex0).sum()) == 0 and int((d1 & ~ex1).sum()) == 0


def test_quirk_case_keeps_far_mutual_matches(gpu_device):
    k0, k1, tr, want0, _ = gt_case("quirk")
    g0, _ = hip_labels(k0.to(gpu_device), k1.to(gpu_device), on(tr, gpu_device), POS, NEG)
    assert torch.equal(g0, want0)
    t0, _ = hip_labels(k0.to(gpu_device), k1.to(gpu_device), on(tr, gpu_device), POS, NEG, apply_thresholds=True)
    assert int((t0 == -1).sum()) > int((g0 == -1).sum())       # with the rules applied the 8 px pairs become unmatched


def test_depth_map_index_out_of_range_raises(gpu_device):
    k0, k1, tr, _, _ = gt_case("depthmap")
    k0 = k0.clone()
    k0[1, 5, 0] = -200.0                                  # int64 -200 < -W: torch raises IndexError
    with pytest.raises(IndexError):
        ref.gt_matches(k0, k1, tr, POS, NEG)
    with pytest.raises(IndexError):
        hip_labels(k0.to(gpu_device), k1.to(gpu_device), on(tr, gpu_device), POS, NEG)
    k1 = k1.clone()
    k1[0, 3, 1] = 60.0                                    # == H: out of range on image 1's map
    with pytest.raises(IndexError):
        hip_labels(gt_case("depthmap")[0].to(gpu_device), k1.to(gpu_device), on(tr, gpu_device), POS, NEG)
    # the device is still fine afterwards
    g0, _ = hip_labels(*(t.to(gpu_device) for t in gt_case("depthmap")[:2]), on(tr, gpu_device), POS, NEG)
    assert torch.equal(g0, gt_case("depthmap")[3])


@pytest.mark.parametrize("B,m,n", [(1, 1, 1), (2, 63, 65), (3, 300, 129), (1, 8192, 8192), (2, 1000, 7)])
def test_label_shapes(gpu_device, B, m, n):
    g = torch.Generator().manual_seed(m * 7 + n)
    k0 = torch.rand(B, m, 2, generator=g) * 1000.0
    k1 = torch.rand(B, n, 2, generator=g) * 1000.0
    Hm = torch.eye(3).repeat(B, 1, 1)
    Hm[:, :2, 2] = torch.randn(B, 2, generator=g)
    tr = {"type": ["perspective"] * B, "H": Hm}
    for apply in (False, True):
        g0, g1 = hip_labels(k0.to(gpu_device), k1.to(gpu_device), on(tr, gpu_device), 3.0, 5.0, apply)
        r0, r1 = ref.gt_matches(k0, k1, tr, 3.0, 5.0, apply_thresholds=apply)
        assert torch.equal(g0, r0) and torch.equal(g1, r1)


def test_no_keypoints_returns_none(gpu_device):
    from openglue_amd import supervision
    tr = {"type": ["perspective"], "H": torch.eye(3, device=gpu_device)[None]}
    k = torch.zeros(1, 0, 2, device=gpu_device)
    assert supervision.generate_gt_matches({"transformation": tr}, feats(k), feats(torch.rand(1, 5, 2, device=gpu_device)), 3.0) == (None, None)


def _crit_inputs(D, dev, grad=True):
    p = f"crit_d{D}"
    S = torch.from_numpy(Z[f"{p}_scores"]).to(dev).requires_grad_(grad)
    a = torch.from_numpy(Z[f"{p}_desc0"]).to(dev).requires_grad_(grad)
    b = torch.from_numpy(Z[f"{p}_desc1"]).to(dev).requires_grad_(grad)
    g0, g1 = torch.from_numpy(Z[f"{p}_gt0"]).to(dev), torch.from_numpy(Z[f"{p}_gt1"]).to(dev)
    return S, a, b, g0, g1


def _rel(got, want):
    return float(np.abs(got - want).max() / max(np.abs(want).max(), 1e-30))


@pytest.mark.parametrize("D", (128, 256))
@pytest.mark.parametrize("margin", (None, 0.2))
def test_criterion_against_reference_and_float64(gpu_device, D, margin):
    from openglue_amd import supervision
    name = f"crit_d{D}_{'none' if margin is None else 'margin'}"
    S, a, b, g0, g1 = _crit_inputs(D, gpu_device)
    lo = supervision.criterion({"gt_matches0": g0, "gt_matches1": g1},
                               {"scores": S, "context_descriptors0": a, "context_descriptors1": b}, margin=margin)
    (lo["loss"] + lo["metric_loss"]).backward()
    assert abs(lo["loss"].item() - float(Z[f"{name}_loss"])) <= 1e-5 * abs(float(Z[f"{name}_loss"]))
    if margin is None:
        assert lo["metric_loss"].item() == 0.0 and a.grad is None and b.grad is None
    else:
        assert abs(lo["metric_loss"].item() - float(Z[f"{name}_metric_loss"])) <= 1e-5 * abs(float(Z[f"{name}_metric_loss"]))
    # float64 autograd of the restatement
    S64, a64, b64 = (t.detach().cpu().double().requires_grad_(True) for t in (S, a, b))
    l64 = ref.criterion(g0.cpu(), g1.cpu(), S64, a64, b64, margin)
    (l64["loss"] + l64["metric_loss"]).backward()
    errs = {"scores": (_rel(S.grad.cpu().numpy(), Z[f"{name}_grad_scores"]), _rel(S.grad.cpu().double().numpy(), S64.grad.numpy()))}
    if margin is not None:
        for key, got, w64 in (("desc0", a.grad, a64.grad), ("desc1", b.grad, b64.grad)):
            errs[key] = (_rel(got.cpu().numpy(), Z[f"{name}_grad_{key}"]), _rel(got.cpu().double().numpy(), w64.numpy()))
    print(f"[{name}] relative gradient errors (vs fixture, vs float64): {errs}")
    for key, (e_fix, e_64) in errs.items():
        assert e_fix < 1e-5 and e_64 < 1e-5, key


def test_criterion_is_deterministic(gpu_device):
    from openglue_amd import supervision
    S, a, b, g0, g1 = _crit_inputs(256, gpu_device, grad=False)
    vals = []
    for _ in range(2):
        lo = supervision.criterion({"gt_matches0": g0, "gt_matches1": g1},
                                   {"scores": S, "context_descriptors0": a, "context_descriptors1": b}, margin=0.2)
        vals.append((lo["loss"].cpu().numpy().tobytes(), lo["metric_loss"].cpu().numpy().tobytes()))
    assert vals[0] == vals[1]


def test_criterion_on_the_train_margin_fixture(gpu_device):
    """The HIP train-mode forward on tests/golden/train_margin.npz's case, then supervision.criterion(margin=...): the stored loss
    and metric_loss of the reference's training step (the forward differs from the reference by fp32 rounding, as in
    tests/test_train_slice.py, hence the looser tolerance there)."""
    from openglue_amd import supervision
    from openglue_amd.superglue import SuperGlue
    from tests.test_train_slice import GM, _margin_case
    cfg, sd, data, gt0, gt1, margin, wn, wm = _margin_case()
    model = SuperGlue(cfg)
    model.load_state_dict(sd)
    model = model.to(gpu_device).train()
    out = model({k: (v.to(gpu_device) if torch.is_tensor(v) else v) for k, v in data.items()})
    lo = supervision.criterion({"gt_matches0": gt0.to(gpu_device), "gt_matches1": gt1.to(gpu_device)}, out, margin=margin)
    assert abs(lo["loss"].item() - float(GM["loss"])) < 1e-3 * abs(float(GM["loss"]))
    assert abs(lo["metric_loss"].item() - float(GM["metric_loss"])) < 1e-3 * abs(float(GM["metric_loss"]))
    (wn * lo["loss"] + wm * lo["metric_loss"]).backward()
    for k, p in model.named_parameters():
        want = GM[f"grad_{k}"]
        got = p.grad.cpu().numpy() if p.grad is not None else np.zeros_like(want)
        if np.abs(want).max() > 1e-7:
            assert _rel(got, want) < 1e-3, k


def test_memory_below_one_dense_buffer(gpu_device):
    from openglue_amd import supervision
    B, M, N, D = 2, 2048, 2048, 256
    g = torch.Generator(device=gpu_device).manual_seed(0)
    k0 = torch.rand(B, M, 2, device=gpu_device, generator=g) * 1000.0
    k1 = torch.rand(B, N, 2, device=gpu_device, generator=g) * 1000.0
    tr = {"type": ["perspective"] * B, "H": torch.eye(3, device=gpu_device).repeat(B, 1, 1)}
    S = torch.randn(B, M + 1, N + 1, device=gpu_device, generator=g).requires_grad_(True)
    a = torch.randn(B, D, M, device=gpu_device, generator=g).requires_grad_(True)
    b = torch.randn(B, D, N, device=gpu_device, generator=g).requires_grad_(True)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    _, y = supervision.generate_gt_matches({"transformation": tr}, feats(k0), feats(k1), 3.0, 5.0)
    lo = supervision.criterion(y, {"scores": S, "context_descriptors0": a, "context_descriptors1": b}, margin=0.2)
    (lo["loss"] + lo["metric_loss"]).backward()
    torch.cuda.synchronize()
    grad_scores = S.grad.numel() * 4
    extra = torch.cuda.max_memory_allocated() - base - grad_scores
    dense = B * M * N * 4
    print(f"[memory] peak increase without grad_scores {extra / 2**20:.2f} MiB; one B*M*N fp32 buffer {dense / 2**20:.2f} MiB")
    assert extra < dense


def test_train_step_example(gpu_device):
    from examples.train_step import run
    for transform in ("perspective", "3d_reprojection"):
        losses, grads = run(steps=6, pairs=2, kpts=256, dim=64, stages=2, lr=1e-3, transform=transform, log=lambda *_: None)
        assert all(np.isfinite(losses)) and losses[-1] < losses[0], (transform, losses)
        missing = [k for k, v in grads.items() if v is None or not bool(torch.isfinite(v).all()) or float(v.abs().max()) == 0.0]
        assert not missing, (transform, missing)
