"""Float64 restatement of SuperPointNetBn with its modules in train() (reference models/features/superpoint/model.py:180-199): every
BatchNorm2d normalises with the statistics of its own input batch (F.batch_norm(training=True)) and moves its running buffers.

dense_train(sd, image) -> heatmap [B, Hc*8, Wc*8], coarse descriptors [B, Hc, Wc, D] (NHWC, unit norm), and the buffers after the call
({"bn1a.running_mean": ..., "bn1a.running_var": ..., "bn1a.num_batches_tracked": ..., ...}); `sd` itself is left unchanged.
Differentiable in the tensors of `sd`.  pool_margins() is the condition the gradient tests put on their inputs."""
from __future__ import annotations

import torch
import torch.nn.functional as F

from openglue_amd import synthetic as syn

# the end-to-end cases of tests/test_gpu_superpoint_bn_train.py; tests/test_superpoint_bn_train_cpu.py checks the conditions on them.
# The image seeds are the ones, of 0..149, at which no pool window's two largest float64 activations lie closer than 1e-5 relative.
CASES = {
    "b2_44x60": dict(B=2, H=44, W=60, seed=39, kw={}),                                 # the third pool drops a row and a column, ragged tiles, N = 70 at the coarse level
    "b1_72x136": dict(B=1, H=72, W=136, seed=140, kw={}),                               # nine tile rows, a half tile column
    "b1_8x16": dict(B=1, H=8, W=16, seed=0, kw=dict(remove_borders_size=0, nms_kernel=3)),   # N = 2 at the coarse level: the smallest legal batch
}


def images(case):
    c = CASES[case]
    return torch.cat([syn.make_image(c["H"], c["W"], seed=c["seed"] + i) for i in range(c["B"])])


TRUNK = [f"{i}{s}" for i in range(1, 5) for s in "ab"]
BN_NAMES = ["bn" + t for t in TRUNK] + ["bnPa", "bnPb", "bnDa", "bnDb"]


def dense_train(sd, image: torch.Tensor, dtype=torch.float64, momentum=0.1, eps=1e-5, taps=None):
    """taps (optional dict): receives every pooled layer's activation before its pool, for pool_margins()."""
    new = {}

    def block(tag, x):
        w, b = sd[f"conv{tag}.weight"].to(dtype), sd[f"conv{tag}.bias"].to(dtype)
        z = F.conv2d(x, w, b, padding=w.shape[-1] // 2)
        rm = sd[f"bn{tag}.running_mean"].detach().to(dtype).clone()
        rv = sd[f"bn{tag}.running_var"].detach().to(dtype).clone()
        y = F.batch_norm(z, rm, rv, sd[f"bn{tag}.weight"].to(dtype), sd[f"bn{tag}.bias"].to(dtype), True, momentum, eps)
        new[f"bn{tag}.running_mean"], new[f"bn{tag}.running_var"] = rm, rv
        new[f"bn{tag}.num_batches_tracked"] = sd[f"bn{tag}.num_batches_tracked"] + 1
        return y

    x = image.to(dtype)
    for i, tag in enumerate(TRUNK):
        x = F.relu(block(tag, x))
        if tag.endswith("b") and i < 6:
            if taps is not None:
                taps[tag] = x
            x = F.max_pool2d(x, 2, 2)
    d = block("Db", F.relu(block("Da", x)))
    d = d / torch.norm(d, p=2, dim=1, keepdim=True)
    s = F.softmax(block("Pb", F.relu(block("Pa", x))), 1)[:, :-1]
    b, _, h, w = s.shape
    heat = s.permute(0, 2, 3, 1).reshape(b, h, w, 8, 8).permute(0, 1, 3, 2, 4).reshape(b, h * 8, w * 8)
    return heat, d.permute(0, 2, 3, 1).contiguous(), new


def pool_margins(taps) -> float:
    """The smallest relative gap between the two largest activations of any 2x2 pool window whose maximum is positive.  A window that
    float64 and fp32 could decide differently moves a whole gradient element; the test inputs are chosen so that there is none."""
    worst = float("inf")
    for a in taps.values():
        B, C, H, W = a.shape
        win = a[:, :, :H // 2 * 2, :W // 2 * 2].reshape(B, C, H // 2, 2, W // 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(B, C, H // 2, W // 2, 4)
        top = torch.topk(win, 2, dim=-1).values
        live = top[..., 0] > 0
        if bool(live.any()):
            worst = min(worst, float(((top[..., 0] - top[..., 1]) / top[..., 0])[live].min()))
    return worst
