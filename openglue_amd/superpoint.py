"""SuperPoint detector and descriptor on HIP kernels: drop-ins for SuperPointNet / SuperPointNetBn of the reference
(models/features/superpoint/model.py).  Inference and fine-tuning (the reference's `finetune: True`) for both.

Same constructor arguments and defaults, same state-dict keys and shapes, same `weights=` loading, and `forward(image, mask=None)`
returns (lafs [B, N, 2, 3], scores [B, N], descriptors [B, N, 256]) -- what features.prepare_features_output and
SuperGlue.match take.  Every step runs in csrc/superpoint.hip (og_superpoint_dense / _detect / _describe): no ATen, MIOpen or
kornia on the path, and no CPU path.

Semantics reproduced: the trunk and heads of model.py (BatchNorm folded into the convolutions at pack time), kornia's nms2d
(replicate padding, strictly greater than the other k*k-1 pixels of the window), F.threshold + nonzero (score > threshold and
!= 0, raster order), remove_borders, top_k_keypoints, min_stack and sample_desc_from_points.  Where torch leaves the order of
equal scores undefined (torch.topk), equal scores are ordered by raster index, lower first.

One device -> host synchronisation per call: the kept count, which sizes the outputs.

Fine-tuning: SuperPointNet.forward in train() mode, with grad enabled and a parameter that requires grad, returns scores and descriptors
with a grad_fn (_SuperPointTrain: csrc/superpoint_train.hip for the ten 3x3 layers and the descriptor sampling, the exact-fp32 GEMM of
train.py for the two 1x1 heads, tensor algebra for the softmax / L2-norm derivatives at coarse resolution).  Same values as eval(), bit
for bit; the selection stays the inference kernels and carries no gradient, as in the reference.

SuperPointNetBn in train() mode (_SuperPointBnTrain, csrc/superpoint_bn_train.hip): every BatchNorm2d normalises with the statistics of
its own batch and moves its running buffers, with grad enabled or not, like nn.BatchNorm2d; scores and descriptors carry a grad_fn
for the 24 convolution and 24 BatchNorm parameters.  The selection runs on the batch-statistics heatmap.  eval() is the folded blob.
"""
from __future__ import annotations

import ctypes as C
import pathlib
from typing import Optional, Union

import torch
import torch.nn as nn

from . import _lib

CONV_NAMES = [f"conv{i}{s}" for i in range(1, 5) for s in "ab"] + ["convPa", "convPb", "convDa", "convDb"]
BN_NAMES = [f"bn{i}{s}" for i in range(1, 5) for s in "ab"] + ["bnPa", "bnPb", "bnDa", "bnDb"]


def _conv2d(ch_in: int, ch_out: int) -> nn.Conv2d:
    return nn.Conv2d(ch_in, ch_out, kernel_size=(3, 3), stride=(1, 1), padding=1)


class SuperPointNet(nn.Module):
    """SuperPoint (https://arxiv.org/abs/1712.07629), reference model.py:15."""

    _batch_norm = False

    def __init__(self, max_keypoints: int = -1, descriptor_dim: int = 256, nms_kernel: int = 9,
                 remove_borders_size: int = 4, keypoint_threshold: float = 0.0,
                 weights: Optional[Union[str, pathlib.Path]] = None):
        super().__init__()
        self.max_keypoints = max_keypoints
        self.descriptor_dim = descriptor_dim
        self.nms_kernel = nms_kernel
        self.remove_borders_size = remove_borders_size
        self.keypoint_threshold = keypoint_threshold
        self.relu = nn.ReLU(inplace=True)
        self.pool = nn.MaxPool2d(kernel_size=2, stride=2)
        self.layers_channels = [[1, 64, 64, 64], [64, 64, 64, 64], [64, 128, 128, 128], [128, 128, 128, 128]]
        for i, ch in enumerate(self.layers_channels):
            setattr(self, f"conv{i + 1}a", _conv2d(ch[0], ch[1]))
            setattr(self, f"conv{i + 1}b", _conv2d(ch[2], ch[3]))
        self.convPa = _conv2d(128, 256)
        self.convPb = nn.Conv2d(256, 65, kernel_size=1, stride=1, padding=0)
        self.convDa = _conv2d(128, 256)
        self.convDb = nn.Conv2d(256, descriptor_dim, kernel_size=1, stride=1, padding=0)
        self._packed: Optional[torch.Tensor] = None
        self._packed_key = None
        self._packed_grad: Optional[torch.Tensor] = None
        self._packed_grad_key = None
        self._packed_raw: Optional[torch.Tensor] = None
        self._packed_raw_key = None
        self.keep_layer_grads = False                # debug: backward leaves the per-layer pre-activation gradients in self.layer_grads
        self.layer_grads = {}
        self._load_weights(weights)

    def _load_weights(self, weights):
        if weights is not None:
            state_dict = torch.load(str(weights), map_location="cpu")
            print(self.load_state_dict(state_dict, strict=True))

    # ---------------------------------------------------------------- packing
    def _pack_tensors(self):
        ts = []
        for n in CONV_NAMES:
            m = getattr(self, n)
            ts += [m.weight, m.bias]
        if self._batch_norm:
            for n in BN_NAMES:
                m = getattr(self, n)
                ts += [m.weight, m.bias, m.running_mean, m.running_var]
        return ts

    def _pack(self, device: torch.device) -> torch.Tensor:
        ts = self._pack_tensors()
        # in-place updates bump _version; storage swaps change data_ptr (as SuperGlue._pack)
        key = (str(device),) + tuple((t.data_ptr(), t._version) for t in ts)
        if self._packed is not None and self._packed_key == key:
            return self._packed
        lib = _lib.load()
        host = [t.detach().to("cpu", torch.float32).contiguous() for t in ts]
        ptrs = (C.c_void_p * len(host))(*[h.data_ptr() for h in host])
        nbytes = lib.og_superpoint_packed_bytes(self.descriptor_dim)
        blob = torch.empty(nbytes, dtype=torch.uint8)
        eps = float(self.bn1a.eps) if self._batch_norm else 0.0
        _lib.check(lib.og_superpoint_pack(self.descriptor_dim, int(self._batch_norm), eps, ptrs, blob.data_ptr()), "og_superpoint_pack")
        self._packed = blob.to(device)
        self._packed_key = key
        return self._packed

    # ---------------------------------------------------------------- checks
    def _check(self, image: torch.Tensor):
        if self._batch_norm and self.training and isinstance(image, torch.Tensor) and not image.is_cuda:
            raise NotImplementedError(f"{type(self).__name__}: no CPU path for training-mode BatchNorm; move the image to the GPU or call .eval()")
        if self.descriptor_dim != 256:
            raise ValueError(f"descriptor_dim must be 256, got {self.descriptor_dim}")
        k = int(self.nms_kernel)
        if k % 2 == 0:
            raise ValueError(f"nms_kernel must be odd, got {k}")
        if not 3 <= k <= 17:
            raise ValueError(f"nms_kernel must be in 3..17, got {k}")
        if self.remove_borders_size < 0:
            raise ValueError(f"remove_borders_size must be >= 0, got {self.remove_borders_size}")
        if not isinstance(image, torch.Tensor) or image.dim() != 4 or image.shape[1] != 1:
            raise ValueError(f"image must be a [B, 1, H, W] tensor, got {getattr(image, 'shape', type(image))}")
        if image.shape[0] < 1 or image.shape[2] // 8 == 0 or image.shape[3] // 8 == 0:
            raise ValueError(f"image {list(image.shape)}: H // 8 and W // 8 must be >= 1")
        if not image.is_cuda:
            raise RuntimeError("SuperPoint: expected an image tensor on the GPU; openglue_amd has no CPU path")
        if self._batch_norm and self.training:
            if image.shape[0] * (image.shape[2] // 8) * (image.shape[3] // 8) < 2:
                raise ValueError(f"image {list(image.shape)}: training-mode BatchNorm needs more than one value per channel "
                                 "(B * (H // 8) * (W // 8) >= 2)")
            for n in BN_NAMES:
                m = getattr(self, n)
                if m.momentum is None or not m.track_running_stats:
                    raise ValueError(f"{n}: training-mode BatchNorm needs a momentum and track_running_stats=True")

    # ---------------------------------------------------------------- stages
    def dense(self, image: torch.Tensor, workspace: Optional[torch.Tensor] = None):
        """-> heatmap [B, Hc*8, Wc*8] (before NMS), coarse descriptors [B, Hc, Wc, 256] (NHWC)."""
        self._check(image)
        B, _, H, W = image.shape
        dev = image.device
        img = image.detach().to(torch.float32).contiguous()
        packed = self._pack(dev)
        Hc, Wc = H // 8, W // 8
        heat = torch.empty(B, Hc * 8, Wc * 8, device=dev, dtype=torch.float32)
        desc = torch.empty(B, Hc, Wc, 256, device=dev, dtype=torch.float32)
        ws = workspace if workspace is not None else self._workspace(B, H, W, dev)
        _lib.call("og_superpoint_dense", dev, B, H, W, img.data_ptr(), packed.data_ptr(), heat.data_ptr(), desc.data_ptr(),
                  ws.data_ptr(), _lib.STREAM)
        return heat, desc

    def _workspace(self, B, H, W, dev) -> torch.Tensor:
        n = _lib.load().og_superpoint_workspace_bytes(B, H, W, int(self.nms_kernel), int(self.max_keypoints))
        if n == 0:
            raise ValueError(f"SuperPoint: unsupported image batch [{B}, 1, {H}, {W}] (B * H * W <= 2^26)")
        return torch.empty(n, device=dev, dtype=torch.uint8)

    def detect(self, heat: torch.Tensor, workspace: torch.Tensor):
        """heatmap -> (counts [2B] int32 on the device, sel_idx [B, cap], sel_score [B, cap], cap)."""
        B, Hh, Wh = heat.shape
        dev = heat.device
        k = int(self.max_keypoints)
        cap = _lib.load().og_superpoint_capacity(Hh, Wh, k)
        counts = torch.empty(2 * B, device=dev, dtype=torch.int32)
        sidx = torch.empty(B, cap, device=dev, dtype=torch.int32)
        sscore = torch.empty(B, cap, device=dev, dtype=torch.float32)
        _lib.call("og_superpoint_detect", dev, B, Hh, Wh, int(self.nms_kernel), int(self.remove_borders_size), float(self.keypoint_threshold),
                  k, heat.data_ptr(), counts.data_ptr(), sidx.data_ptr(), sscore.data_ptr(), cap, workspace.data_ptr(), _lib.STREAM)
        return counts, sidx, sscore, cap

    def describe(self, n: int, sidx: torch.Tensor, sscore: torch.Tensor, desc: torch.Tensor):
        B, Hc, Wc, _ = desc.shape
        dev = desc.device
        lafs = torch.empty(B, n, 2, 3, device=dev, dtype=torch.float32)
        scores = torch.empty(B, n, device=dev, dtype=torch.float32)
        descriptors = torch.empty(B, n, 256, device=dev, dtype=torch.float32)
        _lib.call("og_superpoint_describe", dev, B, Hc, Wc, n, sidx.data_ptr(), sscore.data_ptr(), sidx.shape[1], desc.data_ptr(),
                  lafs.data_ptr(), scores.data_ptr(), descriptors.data_ptr(), _lib.STREAM)
        return lafs, scores, descriptors

    def _differentiable(self) -> bool:
        return self.training and torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters())

    def _pack_grad(self, device: torch.device) -> torch.Tensor:
        """The data-gradient blob (weights transposed, taps flipped), repacked when a weight changes -- as _pack.  It holds the 24
        convolution tensors only: a BatchNorm buffer that moves (every train-mode step of SuperPointNetBn) does not rebuild it."""
        ts = self._pack_tensors()[:2 * len(CONV_NAMES)]
        key = (str(device),) + tuple((t.data_ptr(), t._version) for t in ts)
        if self._packed_grad is not None and self._packed_grad_key == key:
            return self._packed_grad
        lib = _lib.load()
        host = [t.detach().to("cpu", torch.float32).contiguous() for t in ts]
        ptrs = (C.c_void_p * len(host))(*[h.data_ptr() for h in host])
        blob = torch.empty(lib.og_superpoint_train_packed_bytes(self.descriptor_dim), dtype=torch.uint8)
        _lib.check(lib.og_superpoint_train_pack(self.descriptor_dim, ptrs, blob.data_ptr()), "og_superpoint_train_pack")
        self._packed_grad = blob.to(device)
        self._packed_grad_key = key
        return self._packed_grad

    def _pack_raw(self, device: torch.device) -> torch.Tensor:
        """The forward blob of the convolutions alone (no BatchNorm folded in): what the train-mode BatchNorm path convolves with."""
        ts = [t for n in CONV_NAMES for t in (getattr(self, n).weight, getattr(self, n).bias)]
        key = (str(device),) + tuple((t.data_ptr(), t._version) for t in ts)
        if self._packed_raw is not None and self._packed_raw_key == key:
            return self._packed_raw
        lib = _lib.load()
        host = [t.detach().to("cpu", torch.float32).contiguous() for t in ts]
        ptrs = (C.c_void_p * len(host))(*[h.data_ptr() for h in host])
        blob = torch.empty(lib.og_superpoint_packed_bytes(self.descriptor_dim), dtype=torch.uint8)
        _lib.check(lib.og_superpoint_pack(self.descriptor_dim, 0, 0.0, ptrs, blob.data_ptr()), "og_superpoint_pack")
        self._packed_raw = blob.to(device)
        self._packed_raw_key = key
        return self._packed_raw

    def forward(self, image: torch.Tensor, mask=None):
        """image [B, 1, H, W] -> lafs [B, N, 2, 3], scores [B, N], descriptors [B, N, 256] (mask is ignored, as in the reference).
        In train() mode with grad enabled and a parameter that requires grad, scores and descriptors carry a grad_fn."""
        self._check(image)
        if self._batch_norm and self.training:       # batch statistics, running buffers updated: also under torch.no_grad()
            convs = [t for n in CONV_NAMES for t in (getattr(self, n).weight, getattr(self, n).bias)]
            bns = [t for n in BN_NAMES for t in (getattr(self, n).weight, getattr(self, n).bias)]
            return _SuperPointBnTrain.apply(self, image, *convs, *bns)
        if self._differentiable():
            return _SuperPointTrain.apply(self, image, *self._pack_tensors())
        with torch.no_grad():
            B, _, H, W = image.shape
            ws = self._workspace(B, H, W, image.device)
            heat, desc = self.dense(image, ws)
            counts, sidx, sscore, _ = self.detect(heat, ws)
            n = int(counts[B].item())                   # the one synchronisation: every image keeps the same count (min_stack)
            return self.describe(n, sidx, sscore, desc)


# flat gradient buffer of og_superpoint_train_backward: (offset, shape) of weight and bias per entry of CONV_NAMES
def _grad_slices():
    chans = [(1, 64), (64, 64), (64, 64), (64, 64), (64, 128), (128, 128), (128, 128), (128, 128)]
    out, o = {}, 0
    for name, (ci, co) in zip(CONV_NAMES[:8], chans):
        out[name] = ((o, (co, ci, 3, 3)), (o + co * ci * 9, (co,)))
        o += co * ci * 9 + co
    w = 256 * 128 * 9                                # heads: convPa rows 0..255, convDa rows 256..511 of one [512][128][9] block
    out["convPa"] = ((o, (256, 128, 3, 3)), (o + 2 * w, (256,)))
    out["convDa"] = ((o + w, (256, 128, 3, 3)), (o + 2 * w + 256, (256,)))
    return out, o + 2 * w + 512


_GRAD_SLICES, _GRAD_FLOATS = _grad_slices()
_TRUNK = CONV_NAMES[:8]                              # first_layer of og_superpoint_train_backward: index into this list, 8 = heads only


def _softmax65_backward(logit: torch.Tensor, dp: torch.Tensor) -> torch.Tensor:
    """float64 logits [npix, 65] and the gradient dp [npix, 64] of the 64 kept probabilities -> the gradient of the logits, in the
    cancellation-free form _SuperPointTrain.backward describes."""
    npix = logit.shape[0]
    e = torch.exp(logit - logit.max(dim=1, keepdim=True).values)
    zero = torch.zeros(npix, 1, device=logit.device, dtype=torch.float64)
    before = torch.cat([zero, torch.cumsum(e, 1)[:, :-1]], 1)
    after = torch.cat([torch.cumsum(e.flip(1), 1)[:, :-1].flip(1), zero], 1)
    Z = before[:, -1:] + e[:, -1:]
    prob, rest = e / Z, (before + after) / Z
    dp65 = torch.cat([dp, zero], 1)                                                 # the dustbin channel receives no gradient
    pd = prob * dp65
    return prob * (dp65 * rest - (pd.sum(1, keepdim=True) - pd))


# ---- what the backward of SuperPointNet and of SuperPointNetBn share
def _backward_result(names, need, P, grads):
    """The tuple an autograd backward returns for (net, image, weight and bias of `names` in order): a parameter that needs a gradient
    and received none gets zeros."""
    out = []
    for name in names:
        for k in (0, 1):
            g = grads[name][k]
            if need[name][k] and g is None:
                g = torch.zeros_like(P[name][k])
            out.append(g if need[name][k] else None)
    return (None, None, *out)


def _detector_prelude(ops, dscores, sidx, n, hidden, conv_pb, B, Hc, Wc):
    """From the gradient of the scores: dp [npix, 64], the gradient of the 64 kept probabilities of every cell; convPb's weight padded
    to 68 rows (a multiple of 4, for the GEMMs); hP, convPb's input; and convPb's float64 output [npix, 65].  The logits span ~30 units
    where the heatmap is peaked, so one fp32 ulp of a logit is already 1e-6 of a probability: the 256-term products are recomputed as 16
    exact-fp32 GEMMs over 16 channels each and summed in float64."""
    npix, dev = B * Hc * Wc, hidden.device
    dheat = torch.zeros(B, Hc * 8 * Wc * 8, device=dev, dtype=torch.float32)
    dheat.scatter_(1, sidx[:, :n].long(), dscores.to(torch.float32))                 # the kept pixels of an image are distinct
    dp = dheat.view(B, Hc, 8, Wc, 8).permute(0, 1, 3, 2, 4).reshape(npix, 64)
    Wp = torch.zeros(68, 256, device=dev, dtype=torch.float32)
    Wp[:65] = conv_pb[0].detach().view(65, 256)
    hP = hidden[:, :256].contiguous()
    part = ops.gemm_nt(hP.view(npix, 16, 16).permute(1, 0, 2).contiguous(), Wp.view(68, 16, 16).permute(1, 0, 2).contiguous())
    return dp, Wp, hP, part.double().sum(0)[:, :65] + conv_pb[1].detach().to(torch.float32).double()


def _descriptor_prelude(ddesc, sidx, n, desc, nrm, ws_ptr, B, Hc, Wc):
    """From the gradient of the sampled descriptors, through F.normalize + bilinear sampling (kernels) and the per-cell L2 norm (nrm, the
    norm of the raw coarse descriptor): the gradient of the raw coarse descriptor [npix, 256]."""
    npix, dev = B * Hc * Wc, desc.device
    dd = ddesc.to(torch.float32).contiguous()
    dcoarse = torch.empty(B, Hc, Wc, 256, device=dev, dtype=torch.float32)
    _lib.call("og_superpoint_describe_backward", dev, B, Hc, Wc, n, sidx.data_ptr(), sidx.shape[1], desc.data_ptr(), dd.data_ptr(),
              dcoarse.data_ptr(), ws_ptr, _lib.STREAM)
    dn, dc = desc.view(npix, 256), dcoarse.view(npix, 256)
    return (dc - dn * (dn * dc).sum(1, keepdim=True)) / nrm


def _layer_shapes(H, W):
    """(h, w, C) of the gradient planes of layer_grads behind the eight MFMA layers (conv1b .. conv4b, heads)"""
    return [(H // 2 ** s, W // 2 ** s, c) for s, c in ((0, 64), (1, 64), (1, 64), (2, 128), (2, 128), (3, 128), (3, 128), (3, 512))]


def _conv_grad_views(flat, name):
    """(dW, db) of CONV_NAMES entry `name` as views of the flat gradient buffer"""
    (ow, sw), (ob, sb) = _GRAD_SLICES[name]
    return flat[ow:ow + sw[0] * sw[1] * 9].view(sw), flat[ob:ob + sb[0]]


def _layer_grad_views(dbg, names, shapes, B):
    out, o = {}, 0
    for name, (h, w, c) in zip(names, shapes):
        out[name] = dbg[o:o + B * h * w * c].view(B, h, w, c)
        o += B * h * w * c
    return out


class _SuperPointTrain(torch.autograd.Function):
    """SuperPointNet.forward with a backward.  Inputs: the module, the image, then weight and bias of CONV_NAMES in order."""

    @staticmethod
    def forward(ctx, net, image, *params):
        B, _, H, W = image.shape
        dev = image.device
        img = image.detach().to(torch.float32).contiguous()
        packed = net._pack(dev)
        lib = _lib.load()
        nsaved = lib.og_superpoint_train_saved_bytes(B, H, W)
        if nsaved == 0:
            raise ValueError(f"SuperPoint: unsupported image batch [{B}, 1, {H}, {W}] (B * H * W <= 2^26)")
        Hc, Wc = H // 8, W // 8
        saved = torch.empty(nsaved // 4, device=dev, dtype=torch.float32)
        heat = torch.empty(B, Hc * 8, Wc * 8, device=dev, dtype=torch.float32)
        desc = torch.empty(B, Hc, Wc, 256, device=dev, dtype=torch.float32)
        _lib.call("og_superpoint_train_forward", dev, B, H, W, img.data_ptr(), packed.data_ptr(), saved.data_ptr(), heat.data_ptr(),
                  desc.data_ptr(), _lib.STREAM)
        counts, sidx, sscore, _ = net.detect(heat, net._workspace(B, H, W, dev))
        n = int(counts[B].item())
        lafs, scores, descriptors = net.describe(n, sidx, sscore, desc)
        ctx.net, ctx.n, ctx.shape = net, n, (B, H, W)
        ctx.save_for_backward(img, saved, desc, sidx, *params)
        ctx.mark_non_differentiable(lafs)
        return lafs, scores, descriptors

    @staticmethod
    def backward(ctx, _dlafs, dscores, ddesc):
        from . import ops, train                     # train imports this package's modules; keep the import local
        net, n, (B, H, W) = ctx.net, ctx.n, ctx.shape
        img, saved, desc, sidx, *params = ctx.saved_tensors
        need = {name: (ctx.needs_input_grad[2 + 2 * i], ctx.needs_input_grad[3 + 2 * i]) for i, name in enumerate(CONV_NAMES)}
        P = {name: (params[2 * i], params[2 * i + 1]) for i, name in enumerate(CONV_NAMES)}
        dev = img.device
        grads = {name: [None, None] for name in CONV_NAMES}
        if n == 0:                                   # no keypoint: every gradient is zero, nothing to launch
            return _backward_result(CONV_NAMES, need, P, grads)
        Hc, Wc = H // 8, W // 8
        npix = B * Hc * Wc
        hidden = saved[:npix * 512].view(npix, 512)
        ws = torch.empty(_lib.load().og_superpoint_train_workspace_bytes(B, H, W, n), device=dev, dtype=torch.uint8)
        ws_ptr = ws.data_ptr() + (-ws.data_ptr()) % 256
        trunk_first = next((i for i, name in enumerate(_TRUNK) if any(need[name])), 8)
        need_hidden = trunk_first < 8 or any(need["convPa"]) or any(need["convDa"])
        g_hidden = torch.zeros(npix, 512, device=dev, dtype=torch.float32)

        # ---- detector head: scores are heatmap values at the kept pixels -> softmax over 65 -> convPb
        if dscores is not None and (need_hidden or any(need["convPb"])):
            dp, Wp, hP, logit = _detector_prelude(ops, dscores, sidx, n, hidden, P["convPb"], B, Hc, Wc)
            # softmax backward, dlogit_c = p_c (dp_c - s) with s = sum_k p_k dp_k, written so that a peaked cell does not cancel: a kept
            # pixel is a local maximum, often with p_c close to 1, where dp_c - s = dp_c (1 - p_c) - (s - p_c dp_c) loses every digit in
            # the textbook form.  1 - p_c = (the sum of the OTHER exponentials) / Z comes from an exclusive prefix and suffix sum (all
            # terms positive); s - p_c dp_c is exactly 0 when the cell holds one keypoint.  Like the logits, everything up to dlog is
            # float64 tensor algebra at coarse resolution.
            dlog = torch.zeros(npix, 68, device=dev, dtype=torch.float32)
            dlog[:, :65] = _softmax65_backward(logit, dp.double())
            dh, dW, db = train._conv_backward(hP, Wp, dlog, need_hidden, any(need["convPb"]))
            if any(need["convPb"]):
                grads["convPb"] = [dW[:65].reshape(65, 256, 1, 1).contiguous(), db[:65].contiguous()]
            if need_hidden:
                g_hidden[:, :256] = dh

        # ---- descriptor head: F.normalize + bilinear sampling (kernels) -> per-cell L2 norm -> convDb
        if ddesc is not None and (need_hidden or any(need["convDb"])):
            Wd, bd = P["convDb"][0].detach().view(256, 256).contiguous(), P["convDb"][1].detach()
            hD = hidden[:, 256:].contiguous()
            nrm = torch.linalg.vector_norm(ops.gemm_nt(hD, Wd, bd), dim=1, keepdim=True)
            draw = _descriptor_prelude(ddesc, sidx, n, desc, nrm, ws_ptr, B, Hc, Wc)
            dh, dW, db = train._conv_backward(hD, Wd, draw, need_hidden, any(need["convDb"]))
            if any(need["convDb"]):
                grads["convDb"] = [dW.reshape(256, 256, 1, 1), db]
            if need_hidden:
                g_hidden[:, 256:] = dh

        # ---- the ten 3x3 layers
        if need_hidden:
            g_hidden = g_hidden * (hidden > 0)       # ReLU of convPa | convDa
            flat = torch.empty(_GRAD_FLOATS, device=dev, dtype=torch.float32)
            shapes = _layer_shapes(H, W)
            dbg = torch.zeros(sum(B * h * w * c for h, w, c in shapes), device=dev, dtype=torch.float32) if net.keep_layer_grads else None
            _lib.call("og_superpoint_train_backward", dev, B, H, W, img.data_ptr(), net._pack_grad(dev).data_ptr(), saved.data_ptr(),
                      g_hidden.data_ptr(), trunk_first, flat.data_ptr(), _lib.ptr(dbg), ws_ptr, _lib.STREAM)
            for name in _TRUNK[trunk_first:] + ["convPa", "convDa"]:
                grads[name] = list(_conv_grad_views(flat, name))
            if dbg is not None:
                net.layer_grads = _layer_grad_views(dbg, _TRUNK[1:] + ["heads"], shapes, B)
        return _backward_result(CONV_NAMES, need, P, grads)


_BN_TRUNK = BN_NAMES[:8] + ["bnPa", "bnDa"]         # the modules og_superpoint_bn_train_forward normalises with, in its order
_BN_OFFSETS = dict(zip(_BN_TRUNK, [0, 64, 128, 192, 256, 384, 512, 640, 768, 1024]))      # their channels in bn_grads [2][1280]


class _SuperPointBnTrain(torch.autograd.Function):
    """SuperPointNetBn.forward in train() mode: batch statistics in every BatchNorm, running buffers updated, with a backward.
    Inputs: the module, the image, weight and bias of CONV_NAMES in order, then weight and bias of BN_NAMES in order.
    csrc/superpoint_bn_train.hip runs the ten 3x3 layers with their BatchNorms; convPb / convDb are the exact-fp32 GEMM, bnPb / bnDb
    og_batchnorm_train_forward on the [B Hc Wc] token rows (65 channels padded to 68)."""

    @staticmethod
    def forward(ctx, net, image, *params):
        from . import ops, train
        B, _, H, W = image.shape
        dev = image.device
        img = image.detach().to(torch.float32).contiguous()
        lib = _lib.load()
        nsaved = lib.og_superpoint_bn_train_saved_bytes(B, H, W)
        if nsaved == 0:
            raise ValueError(f"SuperPoint: unsupported image batch [{B}, 1, {H}, {W}] (B * H * W <= 2^26)")
        mods = [getattr(net, n) for n in _BN_TRUNK]
        tensors = [t for m in mods for t in (m.weight, m.bias, m.running_mean, m.running_var)]
        for t in tensors + [net.bnPb.running_mean, net.bnPb.running_var, net.bnDb.running_mean, net.bnDb.running_var]:
            if t.device != dev or t.dtype != torch.float32 or not t.is_contiguous():
                raise RuntimeError("SuperPointNetBn: BatchNorm parameters and buffers must be contiguous float32 tensors on the image's device")
        Hc, Wc = H // 8, W // 8
        npix = B * Hc * Wc
        saved = torch.empty(nsaved // 4, device=dev, dtype=torch.float32)
        wsbuf = _lib.workspace(lib.og_superpoint_bn_train_workspace_bytes(B, H, W), dev)
        bn = (C.c_void_p * 40)(*[t.data_ptr() for t in tensors])
        eps = (C.c_float * 10)(*[float(m.eps) for m in mods])
        mom = (C.c_float * 10)(*[float(m.momentum) for m in mods])
        _lib.call("og_superpoint_bn_train_forward", dev, B, H, W, img.data_ptr(), net._pack_raw(dev).data_ptr(), bn, eps, mom,
                  saved.data_ptr(), wsbuf[1], _lib.STREAM)
        hidden = saved[:npix * 512].view(npix, 512)
        cP, cD = params[2 * CONV_NAMES.index("convPb"):][:2], params[2 * CONV_NAMES.index("convDb"):][:2]
        # detector head: convPb, bnPb on 68 channels (the three padding channels are zero and stay out of everything)
        Wp = torch.zeros(68, 256, device=dev, dtype=torch.float32)
        Wp[:65] = cP[0].detach().view(65, 256)
        pad = lambda t, fill: torch.cat([t.detach().to(torch.float32), torch.full((3,), fill, device=dev, dtype=torch.float32)])
        zP = ops.gemm_nt(hidden[:, :256].contiguous(), Wp, pad(cP[1], 0.0))
        rm, rv = pad(net.bnPb.running_mean, 0.0), pad(net.bnPb.running_var, 1.0)
        yP = train.batch_norm_train(zP, pad(net.bnPb.weight, 1.0), pad(net.bnPb.bias, 0.0), rm, rv, float(net.bnPb.momentum), float(net.bnPb.eps))
        net.bnPb.running_mean.copy_(rm[:65])
        net.bnPb.running_var.copy_(rv[:65])
        # descriptor head: convDb, bnDb
        zD = ops.gemm_nt(hidden[:, 256:].contiguous(), cD[0].detach().view(256, 256).contiguous(), cD[1].detach())
        yD, meanD, invD = train.batch_norm_train(zD, net.bnDb.weight.detach(), net.bnDb.bias.detach(), net.bnDb.running_mean, net.bnDb.running_var,
                                                 float(net.bnDb.momentum), float(net.bnDb.eps), return_stats=True)
        heat = torch.empty(B, Hc * 8, Wc * 8, device=dev, dtype=torch.float32)
        desc = torch.empty(B, Hc, Wc, 256, device=dev, dtype=torch.float32)
        _lib.call("og_superpoint_bn_cell_tail", dev, B, Hc, Wc, yP.data_ptr(), 68, yD.data_ptr(), heat.data_ptr(), desc.data_ptr(), _lib.STREAM)
        for n in BN_NAMES:
            getattr(net, n).num_batches_tracked += 1
        # the kernels wrote the running buffers through raw pointers: their _version did not move, so the eval-mode blob (keyed on it)
        # would be served stale
        net._packed = net._packed_key = None
        counts, sidx, sscore, _ = net.detect(heat, net._workspace(B, H, W, dev))
        n = int(counts[B].item())
        lafs, scores, descriptors = net.describe(n, sidx, sscore, desc)
        ctx.net, ctx.n, ctx.shape = net, n, (B, H, W)
        ctx.save_for_backward(img, saved, desc, sidx, zD, torch.linalg.vector_norm(yD, dim=1, keepdim=True), meanD, invD, *params)
        ctx.mark_non_differentiable(lafs)
        return lafs, scores, descriptors

    @staticmethod
    def backward(ctx, _dlafs, dscores, ddesc):
        from . import ops, train
        net, n, (B, H, W) = ctx.net, ctx.n, ctx.shape
        img, saved, desc, sidx, zD, nrm, meanD, invD, *params = ctx.saved_tensors
        names = CONV_NAMES + BN_NAMES
        need = {name: (ctx.needs_input_grad[2 + 2 * i], ctx.needs_input_grad[3 + 2 * i]) for i, name in enumerate(names)}
        P = {name: (params[2 * i], params[2 * i + 1]) for i, name in enumerate(names)}
        dev = img.device
        # a convolution bias that needs a gradient receives zeros: the mean subtraction removes it, its gradient is exactly 0
        grads = {name: [None, None] for name in names}
        if n == 0:                                   # no keypoint: every gradient is zero, nothing to launch
            return _backward_result(names, need, P, grads)
        Hc, Wc = H // 8, W // 8
        npix = B * Hc * Wc
        hidden = saved[:npix * 512].view(npix, 512)
        wants = lambda *ns: any(any(need[x]) for x in ns)
        trunk_first = next((i for i, (c, b) in enumerate(zip(_TRUNK, BN_NAMES[:8])) if wants(c, b)), 8)
        need_hidden = trunk_first < 8 or wants("convPa", "convDa", "bnPa", "bnDa")
        g_hidden = torch.zeros(npix, 512, device=dev, dtype=torch.float32)

        # ---- detector head: scores -> softmax over 65 -> bnPb -> convPb, in float64 tensor algebra at coarse resolution
        if dscores is not None and (need_hidden or wants("convPb", "bnPb")):
            dp, Wp, hP, z = _detector_prelude(ops, dscores, sidx, n, hidden, P["convPb"], B, Hc, Wc)
            gam, bet = P["bnPb"][0].detach().double(), P["bnPb"][1].detach().double()
            r = torch.rsqrt(z.var(0, unbiased=False) + float(net.bnPb.eps))
            xh = (z - z.mean(0)) * r
            dy = _softmax65_backward(xh * gam + bet, dp.double())
            dbeta, dgamma = dy.sum(0), (dy * xh).sum(0)
            dz = torch.zeros(npix, 68, device=dev, dtype=torch.float32)
            dz[:, :65] = gam * r * (dy - dbeta / npix - xh * (dgamma / npix))
            dh, dW, _ = train._conv_backward(hP, Wp, dz, need_hidden, need["convPb"][0])
            grads["bnPb"] = [dgamma.to(torch.float32), dbeta.to(torch.float32)]
            if need["convPb"][0]:
                grads["convPb"][0] = dW[:65].reshape(65, 256, 1, 1).contiguous()
            if need_hidden:
                g_hidden[:, :256] = dh

        # ---- descriptor head: F.normalize + bilinear sampling (kernels) -> per-cell L2 norm -> bnDb (og_batchnorm_train_backward) -> convDb
        if ddesc is not None and (need_hidden or wants("convDb", "bnDb")):
            wsd = _lib.workspace(B * n * 264 * 4 + 256, dev)
            dy = _descriptor_prelude(ddesc, sidx, n, desc, nrm, wsd[1], B, Hc, Wc).contiguous()
            dz = torch.empty_like(dy)
            dgamma = torch.empty(256, device=dev, dtype=torch.float32)
            dbeta = torch.empty(256, device=dev, dtype=torch.float32)
            wsb = train._ws(zD, npix, 256)
            _lib.call("og_batchnorm_train_backward", dev, zD.data_ptr(), 256, dy.data_ptr(), 256, npix, 256, P["bnDb"][0].detach().data_ptr(),
                      meanD.data_ptr(), invD.data_ptr(), 0, dz.data_ptr(), 256, dgamma.data_ptr(), dbeta.data_ptr(), wsb.data_ptr(), _lib.STREAM)
            hD = hidden[:, 256:].contiguous()
            dh, dW, _ = train._conv_backward(hD, P["convDb"][0].detach().view(256, 256).contiguous(), dz, need_hidden, need["convDb"][0])
            grads["bnDb"] = [dgamma, dbeta]
            if need["convDb"][0]:
                grads["convDb"][0] = dW.reshape(256, 256, 1, 1)
            if need_hidden:
                g_hidden[:, 256:] = dh

        # ---- the ten 3x3 layers and their BatchNorms
        if need_hidden:
            flat = torch.empty(_GRAD_FLOATS, device=dev, dtype=torch.float32)
            bnflat = torch.zeros(2, 1280, device=dev, dtype=torch.float32)
            shapes = [(H, W, 64)] + _layer_shapes(H, W)                              # bn1a's dz first
            dbg = torch.zeros(sum(B * h * w * c for h, w, c in shapes), device=dev, dtype=torch.float32) if net.keep_layer_grads else None
            wsbuf = _lib.workspace(_lib.load().og_superpoint_bn_train_workspace_bytes(B, H, W), dev)
            _lib.call("og_superpoint_bn_train_backward", dev, B, H, W, img.data_ptr(), net._pack_grad(dev).data_ptr(), saved.data_ptr(),
                      g_hidden.data_ptr(), trunk_first, flat.data_ptr(), bnflat.data_ptr(), _lib.ptr(dbg), wsbuf[1], _lib.STREAM)
            for name in _TRUNK[trunk_first:] + ["convPa", "convDa"]:
                grads[name][0] = _conv_grad_views(flat, name)[0]
            for name in _BN_TRUNK[trunk_first:]:
                o, c = _BN_OFFSETS[name], getattr(net, name).num_features
                grads[name] = [bnflat[0, o:o + c], bnflat[1, o:o + c]]
            if dbg is not None:
                net.layer_grads = _layer_grad_views(dbg, _TRUNK + ["heads"], shapes, B)
        return _backward_result(names, need, P, grads)


class SuperPointNetBn(SuperPointNet):
    """SuperPoint with BatchNorm after every convolution (reference model.py:129).  eval(): the BatchNorms folded into the convolutions
    at pack time.  train(): batch statistics, running buffers updated, differentiable (_SuperPointBnTrain)."""

    _batch_norm = True

    def __init__(self, max_keypoints: int = -1, descriptor_dim: int = 256, nms_kernel: int = 9,
                 remove_borders_size: int = 4, keypoint_threshold: float = 0.0,
                 weights: Optional[Union[str, pathlib.Path]] = None):
        super().__init__(max_keypoints, descriptor_dim, nms_kernel, remove_borders_size, keypoint_threshold, weights=None)
        for i, ch in enumerate(self.layers_channels):
            setattr(self, f"bn{i + 1}a", nn.BatchNorm2d(ch[1]))
            setattr(self, f"bn{i + 1}b", nn.BatchNorm2d(ch[3]))
        self.bnPa = nn.BatchNorm2d(256)
        self.bnPb = nn.BatchNorm2d(65)
        self.bnDa = nn.BatchNorm2d(256)
        self.bnDb = nn.BatchNorm2d(256)
        self._load_weights(weights)

    @staticmethod
    def rename_weights_keys(state_dict):
        """pytorch-superpoint checkpoint keys -> this module's (reference model.py:150-170)."""
        pairs = [("inc.conv.conv.0", "conv1a"), ("inc.conv.conv.1", "bn1a"), ("inc.conv.conv.3", "conv1b"), ("inc.conv.conv.4", "bn1b")]
        for i in range(1, 4):
            for src, dst in ((0, "a"), (1, "a"), (3, "b"), (4, "b")):
                pairs.append((f"down{i}.mpconv.1.conv.{src}", f"{'conv' if src in (0, 3) else 'bn'}{i + 1}{dst}"))
        for key in list(state_dict.keys()):
            new = key
            for a, b in pairs:
                new = new.replace(a, b)
            state_dict[new] = state_dict.pop(key)
        return state_dict

    def _load_weights(self, weights):
        if weights is not None:
            state_dict = torch.load(str(weights), map_location="cpu")["model_state_dict"]
            state_dict = self.rename_weights_keys(state_dict)
            print(self.load_state_dict(state_dict, strict=True))


methods = {"SuperPointNet": SuperPointNet, "SuperPointNetBn": SuperPointNetBn}
