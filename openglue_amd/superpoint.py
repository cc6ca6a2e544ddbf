"""SuperPoint detector and descriptor on HIP kernels: drop-ins for SuperPointNet / SuperPointNetBn of the reference
(models/features/superpoint/model.py), inference only.

Same constructor arguments and defaults, same state-dict keys and shapes, same `weights=` loading, and `forward(image, mask=None)`
returns (lafs [B, N, 2, 3], scores [B, N], descriptors [B, N, 256]) -- what features.prepare_features_output and
SuperGlue.match take.  Every step runs in csrc/superpoint.hip (og_superpoint_dense / _detect / _describe): no ATen, MIOpen or
kornia on the path, and no CPU path.

Semantics reproduced: the trunk and heads of model.py (BatchNorm folded into the convolutions at pack time), kornia's nms2d
(replicate padding, strictly greater than the other k*k-1 pixels of the window), F.threshold + nonzero (score > threshold and
!= 0, raster order), remove_borders, top_k_keypoints, min_stack and sample_desc_from_points.  Where torch leaves the order of
equal scores undefined (torch.topk), equal scores are ordered by raster index, lower first.

One device -> host synchronisation per call: the kept count, which sizes the outputs.
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
        if self._batch_norm and self.training:
            raise NotImplementedError(f"{type(self).__name__}: training-mode BatchNorm is not supported; call .eval()")
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

    @torch.no_grad()
    def forward(self, image: torch.Tensor, mask=None):
        """image [B, 1, H, W] -> lafs [B, N, 2, 3], scores [B, N], descriptors [B, N, 256] (mask is ignored, as in the reference)."""
        self._check(image)
        B, _, H, W = image.shape
        ws = self._workspace(B, H, W, image.device)
        heat, desc = self.dense(image, ws)
        counts, sidx, sscore, _ = self.detect(heat, ws)
        n = int(counts[B].item())                   # the one synchronisation: every image keeps the same count (min_stack)
        return self.describe(n, sidx, sscore, desc)


class SuperPointNetBn(SuperPointNet):
    """SuperPoint with BatchNorm after every convolution (reference model.py:129); eval mode only."""

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
