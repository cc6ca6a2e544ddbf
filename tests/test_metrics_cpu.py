"""CPU checks of the validation metrics (openglue_amd.metrics): the AUC rule of CameraPoseAUC.compute against the float64
restatement in tests/metrics_ref.py, the restatement itself on constructed geometry, the wrappers' refusal of CPU tensors, and
the register / scratch budget of csrc/metrics.hip as the compiler reports it for gfx950."""
import math
import os
import re
import shutil
import subprocess

import pytest
import torch

from openglue_amd import metrics
from tests import metrics_ref as ref

THRESHOLDS = [5.0, 10.0, 20.0]
ERROR_LISTS = {
    "with_inf": [0.5, 3.0, math.inf, 7.5, math.inf, 15.0],
    "ties": [2.0, 2.0, 2.0, 8.0, 8.0, 30.0],
    "at_thresholds": [5.0, 10.0, 20.0, 1.0],
    "all_below": [0.1, 0.2, 0.3, 4.9],
    "none_below": [25.0, 40.0, math.inf],
    "single": [0.0],
}


@pytest.mark.parametrize("name", sorted(ERROR_LISTS))
def test_pose_auc_matches_restatement(name):
    errs = ERROR_LISTS[name]
    got = metrics.pose_auc(torch.tensor(errs, dtype=torch.float32), THRESHOLDS)
    want = ref.pose_auc(errs, THRESHOLDS)
    assert list(got) == ["AUC@5.0deg", "AUC@10.0deg", "AUC@20.0deg"] == list(want)
    for k in want:
        assert abs(float(got[k]) - want[k]) < 1e-6, (k, float(got[k]), want[k])


def test_pose_auc_hand_values():
    got = ref.pose_auc([0.0, 10.0], [5.0])           # recall 0.5 from 0 up to 5: area 0.5 * 5 / 5
    assert abs(got["AUC@5.0deg"] - 0.5) < 1e-12
    assert ref.pose_auc([30.0, math.inf], [5.0])["AUC@5.0deg"] == 0.0
    assert ref.pose_auc([0.0, 0.0], [5.0])["AUC@5.0deg"] == 1.0


def _pose(angle_deg=12.0):
    a = math.radians(angle_deg)
    R = torch.tensor([[math.cos(a), 0.0, math.sin(a)], [0.0, 1.0, 0.0], [-math.sin(a), 0.0, math.cos(a)]], dtype=torch.float64)
    T = torch.tensor([1.0, 0.2, 0.1], dtype=torch.float64)
    K = torch.tensor([[800.0, 0.0, 320.0], [0.0, 780.0, 240.0], [0.0, 0.0, 1.0]], dtype=torch.float64)
    return R, T, K


def test_points_on_epipolar_lines_give_zero():
    R, T, K = _pose()
    g = torch.Generator().manual_seed(0)
    X = torch.rand(50, 3, generator=g, dtype=torch.float64) * torch.tensor([2.0, 2.0, 4.0]) + torch.tensor([-1.0, -1.0, 4.0])
    x0 = X[:, :2] / X[:, 2:]
    Y = X @ R.T + T
    x1 = Y[:, :2] / Y[:, 2:]
    d = ref.symmetrical_epipolar_distance(x0, x1, ref.essential_from_Rt(R, T))
    assert float(d.abs().max()) < 1e-25
    # through the pixel path and the matches layout
    k0 = x0 * K[[0, 1], [0, 1]] + K[:2, 2]
    k1 = x1 * K[[0, 1], [0, 1]] + K[:2, 2]
    dist, mask = ref.epipolar_distances(k0, k1, torch.arange(50), K, K, R, T)
    assert bool(mask.all()) and float(dist.max()) < 1e-20


def test_known_offset_by_hand():
    # pure translation along x: E = [t]x, epipolar lines in both images are horizontal (y = const).  A point moved by dy
    # off its line: x1^T E x0 = -dy (t = (1, 0, 0)), (E x0)_01 = (0, -1), (E^T x1)_01 = (0, 1) -> d = dy^2 (1 + 1)
    R = torch.eye(3, dtype=torch.float64)
    T = torch.tensor([1.0, 0.0, 0.0], dtype=torch.float64)
    E = ref.essential_from_Rt(R, T)
    x0 = torch.tensor([[0.3, 0.1]], dtype=torch.float64)
    dy = 0.01
    x1 = torch.tensor([[0.1, 0.1 + dy]], dtype=torch.float64)
    d = float(ref.symmetrical_epipolar_distance(x0, x1, E)[0])
    assert abs(d - 2 * dy * dy) < 1e-15
    c, p, s = ref.precision_counts(torch.tensor([1e-4, 1e-3, 4.9e-4]), 10, 5e-4)
    assert (c, p, s) == (2, 2 / 3, 0.2)
    assert ref.precision_counts(torch.zeros(0), 10, 5e-4) == (0, 0.0, 0.0)


def test_pose_errors_and_threshold_by_hand():
    R, T, K = _pose(0.0)
    assert ref.rotation_error(R, R) == 0.0
    R2, _, _ = _pose(7.0)
    assert abs(ref.rotation_error(R, R2) - 7.0) < 1e-9
    assert ref.translation_error(T, -T) < 1e-5           # the sign of t is not observable (acos near -1: ~1e-6 deg)
    assert abs(ref.translation_error(torch.tensor([1.0, 0, 0]), torch.tensor([1.0, 1.0, 0])) - 45.0) < 1e-9
    assert abs(ref.pose_error(R, T, R2, T) - 7.0) < 1e-9
    K1 = K.clone()
    K1[0, 0], K1[1, 1] = 1200.0, 1180.0
    assert abs(ref.ransac_threshold(1.0, K, K1) - 2.0 / ((800 + 1200 + 780 + 1180) / 2)) < 1e-9


def test_wrappers_reject_cpu_tensors():
    k = torch.zeros(1, 8, 2)
    m = torch.zeros(1, 8, dtype=torch.int64)
    tr = {"K0": torch.eye(3)[None], "K1": torch.eye(3)[None], "R": torch.eye(3)[None], "T": torch.ones(1, 3)}
    with pytest.raises(RuntimeError, match="GPU"):
        metrics.epipolar_precision(k, k, m, tr)
    with pytest.raises(RuntimeError, match="GPU"):
        metrics.relative_pose(k, k, m, tr, 1.0)
    acc = metrics.AccuracyUsingEpipolarDist()
    with pytest.raises(RuntimeError, match="GPU"):
        acc.update(k[0], k[0], {key: v[0] for key, v in tr.items()}, 8)
    auc = metrics.CameraPoseAUC(THRESHOLDS, 1.0)
    with pytest.raises(RuntimeError, match="GPU"):
        auc.update_batch(k, k, m, tr)


def _hipcc():
    for c in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if c and os.path.exists(c):
            return c
    pytest.fail("hipcc not found")


def test_metrics_kernels_do_not_spill(tmp_path):
    src = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "openglue_amd", "csrc", "metrics.hip")
    r = subprocess.run([_hipcc(), "--offload-arch=gfx950", "-std=c++17", "-O3", "-Rpass-analysis=kernel-resource-usage",
                        "--cuda-device-only", "-c", src, "-o", str(tmp_path / "m.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    usage, name = {}, None
    for line in r.stderr.splitlines():
        mm = re.search(r"Function Name: (\S+)", line)
        if mm:
            name = mm.group(1)
        mm = re.search(r"(VGPRs|ScratchSize \[bytes/lane\]): (\d+)", line)
        if mm and name:
            usage.setdefault(name, {})[mm.group(1)] = int(mm.group(2))
    print({k: v for k, v in usage.items()})
    for kernel in ("score_kernel", "finish_kernel"):
        hits = [v for k, v in usage.items() if kernel in k]
        assert hits and all(v["ScratchSize [bytes/lane]"] == 0 for v in hits), (kernel, usage)
    assert any("solve_poly_kernel" in k for k in usage) and any("solve_roots_kernel" in k for k in usage)
