"""The training step's supervision on HIP kernels: the two pieces of the reference's `training_step` either side of the matcher
(models/matching_module.py:83-105).

  generate_gt_matches   models/gt_matches_generation.py  keypoints + known transformation -> gt_matches0 / gt_matches1
  criterion             utils/losses.py                   y_true, y_pred -> {'loss', 'metric_loss'}, differentiable

Thin wrappers over og_gt_matches / og_criterion_forward / og_criterion_backward (include/openglue_amd.h, csrc/supervision.hip);
GPU tensors only, like features.py.  Neither forms a B x M x N matrix.

The reference's distance thresholds never change a label.  Its lines
    gt_matches0[cross_check_consistent0][symmetric_dist > positive_threshold] = IGNORE_INDEX
(and the four like it, plus the rule "also ignore a MATCHED point whose neighbour has no depth") write into `gt[mask]`, which
is a copy, so the writes are lost.  What it actually returns is

    gt0[i] = nn0[i] if nn1[nn0[i]] == i else -1
    gt0[i] = -2     if keypoint i of image 0 has no depth (|depth| <= 1e-8; never for a homography)
    (image 1 the same way, with the inverse transformation)

and that is the default here (`apply_thresholds=False`): parity with the reference.  `apply_thresholds=True` runs the same
statements as in-place writes with combined masks, in source order -- the behaviour the reference's docstring table describes:
a mutual pair (i, j) with symmetric distance 0.5 (d0[i] + d1[j]) above `positive_threshold` is ignored (-2), above
`negative_threshold` unmatched (-1); a non-mutual keypoint within `negative_threshold` of its nearest neighbour is ignored; a
keypoint without depth is ignored, and so is a mutual keypoint whose neighbour has no depth.  (The reference pairs the
distances of its k-th mutual keypoint of image 0 with the k-th of image 1; here each mutual pair uses its own two distances.)
"""
from __future__ import annotations

from typing import Any, Dict, Optional, Tuple

import torch

from . import _lib

UNMATCHED_INDEX = -1
IGNORE_INDEX = -2
_TRANSFORMS = {"perspective": 0, "3d_reprojection": 1}


def generate_gt_matches(data: Dict[str, Any], features0: Dict[str, torch.Tensor], features1: Dict[str, torch.Tensor],
                        positive_threshold: float, negative_threshold: Optional[float] = None, apply_thresholds: bool = False
                        ) -> Tuple[Optional[Dict[str, Any]], Optional[Dict[str, torch.Tensor]]]:
    """models/gt_matches_generation.py:17-96 on the GPU.  Returns (data merged with keypoints*, local_descriptors*, side_info*,
    {'gt_matches0' [B, M], 'gt_matches1' [B, N]} int64), or (None, None) when either image has no keypoints.  The thresholds only
    act under `apply_thresholds` (see the module docstring).  Raises ValueError for an unknown transformation type and
    IndexError when a keypoint falls outside a depth map (both as the reference does); the latter check waits for the GPU."""
    if negative_threshold is None:
        negative_threshold = positive_threshold
    transformation = data["transformation"]
    ttype = transformation["type"][0]
    if ttype not in _TRANSFORMS:
        raise ValueError(f"Unknown transformation type {ttype}.")
    kpts0 = _lib.gpu_tensor(features0["keypoints"], "features0['keypoints']", convert=True)
    kpts1 = _lib.gpu_tensor(features1["keypoints"], "features1['keypoints']", convert=True)
    B, M = kpts0.shape[:2]
    N = kpts1.shape[1]
    if M == 0 or N == 0:
        return None, None
    if kpts0.shape != (B, M, 2) or kpts1.shape != (B, N, 2):
        raise ValueError("keypoints must be [B, N, 2] with the same B on both sides")
    dev = kpts0.device
    lib = _lib.load()
    keep = []

    def mat(name, shape):
        t = _lib.gpu_tensor(transformation[name], f"transformation['{name}']", convert=True)
        if tuple(t.shape) != shape:
            raise ValueError(f"transformation['{name}'] must be {list(shape)}, got {list(t.shape)}")
        keep.append(t)
        return t.data_ptr()

    H = K0 = K1 = R = T = dp0 = dp1 = None
    dims = [0, 0, 0, 0]
    if ttype == "perspective":
        H = mat("H", (B, 3, 3))
    else:
        K0, K1, R, T = mat("K0", (B, 3, 3)), mat("K1", (B, 3, 3)), mat("R", (B, 3, 3)), mat("T", (B, 3))
        ptrs = []
        for side, cnt in ((0, M), (1, N)):
            d = _lib.gpu_tensor(transformation[f"depth{side}"], f"transformation['depth{side}']", convert=True)
            if d.dim() == 2:
                if tuple(d.shape) != (B, cnt):
                    raise ValueError(f"per-keypoint depth{side} must be [B, {cnt}]")
            elif d.dim() == 3 and d.shape[0] == B and d.shape[1] > 0 and d.shape[2] > 0:
                dims[2 * side], dims[2 * side + 1] = int(d.shape[1]), int(d.shape[2])
            else:
                raise ValueError(f"depth{side} must be [B, N] or a depth map [B, H, W]")
            keep.append(d)
            ptrs.append(d.data_ptr())
        dp0, dp1 = ptrs
    gt0 = torch.empty(B, M, device=dev, dtype=torch.int64)
    gt1 = torch.empty(B, N, device=dev, dtype=torch.int64)
    status = torch.empty(1, device=dev, dtype=torch.int32)
    ws, wp = _lib.workspace(lib.og_gt_matches_workspace_bytes(B, M, N), dev)
    _lib.call("og_gt_matches", dev, B, M, N, kpts0.data_ptr(), kpts1.data_ptr(), _TRANSFORMS[ttype], H, K0, K1, R, T,
              dp0, dims[0], dims[1], dp1, dims[2], dims[3], int(bool(apply_thresholds)),
              float(positive_threshold), float(negative_threshold), gt0.data_ptr(), gt1.data_ptr(),
              status.data_ptr(), wp, _lib.STREAM)
    if dims[0] or dims[2]:
        bad = int(status.item())
        if bad:
            side = 0 if bad & 1 else 1
            raise IndexError(f"keypoints{side} index outside depth{side} of shape {dims[2 * side]} x {dims[2 * side + 1]}")
    data = {
        **data,
        "keypoints0": features0["keypoints"], "keypoints1": features1["keypoints"],
        "local_descriptors0": features0["local_descriptors"], "local_descriptors1": features1["local_descriptors"],
        "side_info0": features0["side_info"], "side_info1": features1["side_info"],
    }
    return data, {"gt_matches0": gt0, "gt_matches1": gt1}


class _Criterion(torch.autograd.Function):
    @staticmethod
    def forward(ctx, scores, desc0, desc1, gt0, gt1, margin):
        lib = _lib.load()
        dev = scores.device
        B, M1, N1 = scores.shape
        M, N = M1 - 1, N1 - 1
        S = _lib.gpu_tensor(scores, "scores", convert=True)
        g0 = _lib.gpu_tensor(gt0, "gt_matches0", torch.int64, convert=True)
        g1 = _lib.gpu_tensor(gt1, "gt_matches1", torch.int64, convert=True)
        if g0.shape != (B, M) or g1.shape != (B, N):
            raise ValueError("gt_matches0 / gt_matches1 must be [B, M] / [B, N] for scores [B, M+1, N+1]")
        on = margin is not None
        D = 0
        a = b = None
        if on:
            a = _lib.gpu_tensor(desc0, "context_descriptors0", convert=True)
            b = _lib.gpu_tensor(desc1, "context_descriptors1", convert=True)
            D = a.shape[1]
            if a.shape != (B, D, M) or b.shape != (B, D, N):
                raise ValueError("context_descriptors0 / 1 must be [B, D, M] / [B, D, N]")
        ws, wp = _lib.workspace(lib.og_criterion_workspace_bytes(B, M, N, int(on)), dev)
        out = torch.empty(2, device=dev, dtype=torch.float32)
        _lib.call("og_criterion_forward", dev, S.data_ptr(), g0.data_ptr(), g1.data_ptr(), _lib.ptr(a), _lib.ptr(b), B, M, N, D, int(on),
                  float(margin) if on else 0.0, out.data_ptr(), wp, _lib.STREAM)
        ctx.keep = (ws, wp, g0, g1, a, b)
        ctx.args = (B, M, N, D, on, float(margin) if on else 0.0)
        ctx.meta = (scores.dtype, desc0.dtype if on else None, desc1.dtype if on else None)
        return out[0].clone(), out[1].clone()

    @staticmethod
    def backward(ctx, g_loss, g_metric):
        ws, wp, g0, g1, a, b = ctx.keep
        B, M, N, D, on, margin = ctx.args
        dev = g0.device
        need_s = ctx.needs_input_grad[0]
        need_d = on and (ctx.needs_input_grad[1] or ctx.needs_input_grad[2])
        if not need_s and not need_d:
            return None, None, None, None, None, None
        zero = torch.zeros((), device=dev, dtype=torch.float32)
        gl = torch.stack([zero if g_loss is None else g_loss.to(torch.float32).reshape(()),
                          zero if g_metric is None else g_metric.to(torch.float32).reshape(())]).contiguous()
        gS = torch.empty(B, M + 1, N + 1, device=dev, dtype=torch.float32) if need_s else None
        gA = torch.empty(B, D, M, device=dev, dtype=torch.float32) if need_d else None
        gB = torch.empty(B, D, N, device=dev, dtype=torch.float32) if need_d else None
        _lib.call("og_criterion_backward", dev, g0.data_ptr(), g1.data_ptr(), _lib.ptr(a), _lib.ptr(b), B, M, N, D, int(on), margin,
                  gl.data_ptr(), wp, _lib.ptr(gS), _lib.ptr(gA), _lib.ptr(gB), _lib.STREAM)
        sd, d0d, d1d = ctx.meta
        return (gS.to(sd) if gS is not None else None, gA.to(d0d) if gA is not None else None,
                gB.to(d1d) if gB is not None else None, None, None, None)


def criterion(y_true: Dict[str, torch.Tensor], y_pred: Dict[str, torch.Tensor], margin: Optional[float] = None
              ) -> Dict[str, torch.Tensor]:
    """utils/losses.py:7-52 on the GPU: {'loss': the NLL over `scores` (dustbins included), 'metric_loss': the triplet / hinge
    loss on the cosine distance of `context_descriptors0/1` (a zero tensor when `margin` is None, and no Gram matrix is
    formed)}.  Gradients flow to `scores` and, with a margin, to both descriptor tensors.  Loss values are bit-identical from
    run to run; the descriptor gradients are float-atomic sums.  Two degenerate inputs follow the reference too: an all-zero
    descriptor (F.normalize clamps it to 0) is at distance 0.25 from every other descriptor and 0 from another zero one, and a
    match that is the only entry of its row or column (M == 1 or N == 1) contributes exactly `margin`, without gradient."""
    scores = y_pred["scores"]
    if not isinstance(scores, torch.Tensor) or not scores.is_cuda:
        raise RuntimeError("scores: expected a tensor on the GPU; openglue_amd has no CPU path")
    d0 = y_pred.get("context_descriptors0")
    d1 = y_pred.get("context_descriptors1")
    if margin is None:
        d0 = d1 = scores.new_zeros(())      # placeholders: not read, no gradient
    loss, metric = _Criterion.apply(scores, d0, d1, y_true["gt_matches0"], y_true["gt_matches1"], margin)
    return {"loss": loss, "metric_loss": metric}
