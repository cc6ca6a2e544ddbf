"""DoG + AffNet + OriNet + HardNet on HIP kernels: a drop-in for the reference's `OPENCVDoGAffNetHardNet`
(models/features/opencv/dog_affnet_harnet.py, config/features/dog_opencv_affnet_hardnet.yaml), inference only.

    lafs, responses = DoG detector                    (openglue_amd/sift.py: pyramid / detect / orient / select / gather)
    lafs = orinet(affnet(lafs, image), image)         (kornia LAFAffNetShapeEstimator(preserve_orientation=True), LAFOrienter(32, OriNet))
    patches = extract_patches_from_pyramid(image, lafs, PS=32)
    descriptors = hardnet(patches)

`forward(image [B, 1, H, W], mask=None)` returns (lafs [B, N, 2, 3], scores [B, N], descriptors [B, N, 128]) on the GPU; the LAFs
carry a real affine shape, which features.prepare_features_output(method="affine") turns into six side channels.  Everything after
the detector runs in csrc/patchnet.hip (og_patch_pyramid / og_patch_extract / og_patchnet_forward): no ATen, MIOpen or kornia on the
path, and no CPU path.  The arithmetic is a kornia 0.6-era reading pinned by tests/patchnet_ref.py; DESIGN.md section 4.12 lists the
known differences.  State-dict keys are kornia's (`hardnet.features.*`, `affnet.features.*`, `orinet.angle_detector.features.*`).

One device -> host synchronisation per call: the detector's counts, which size the outputs.
"""
from __future__ import annotations

import ctypes as C
from typing import List, Optional, Tuple

import torch
import torch.nn as nn

from . import _lib
from .sift import SIFT, geometry as sift_geometry

PS = 32
KINDS = {"hardnet": 0, "affnet": 1, "orinet": 2}
CONV_IDX = (0, 3, 6, 9, 12, 15)


def patchnet_features(kind: str) -> nn.Sequential:
    """kornia's `features` Sequential of HardNet / AffNet / OriNet: convolutions at 0, 3, 6, 9, 12, 15, 19, BatchNorm(affine=False)
    behind each hidden one, Dropout at 18"""
    c = 32 if kind == "hardnet" else 16
    chans = [(1, c, 1), (c, c, 1), (c, 2 * c, 2), (2 * c, 2 * c, 1), (2 * c, 4 * c, 2), (4 * c, 4 * c, 1)]
    layers: List[nn.Module] = []
    for cin, cout, stride in chans:
        layers += [nn.Conv2d(cin, cout, kernel_size=3, stride=stride, padding=1, bias=False), nn.BatchNorm2d(cout, affine=False), nn.ReLU()]
    layers.append(nn.Dropout(0.3 if kind == "hardnet" else 0.25))
    if kind == "hardnet":
        layers += [nn.Conv2d(4 * c, 128, kernel_size=8, bias=False), nn.BatchNorm2d(128, affine=False)]
    else:
        layers += [nn.Conv2d(4 * c, 3 if kind == "affnet" else 2, kernel_size=8, stride=1, padding=0, bias=True), nn.Tanh()]
    return nn.Sequential(*layers)


def pyramid_geometry(H: int, W: int) -> Tuple[List[Tuple[int, int]], int]:
    """-> [(h, w) of every level built], floats per image"""
    out = (C.c_int32 * 26)()
    _lib.check(_lib.load().og_patch_geometry(H, W, out), "og_patch_geometry")
    return [(out[2 + 2 * l], out[3 + 2 * l]) for l in range(out[0])], out[1]


def _scratch(B: int, H: int, W: int, n: int, dev) -> torch.Tensor:
    nbytes = _lib.load().og_patch_workspace_bytes(B, H, W, n)
    if nbytes == 0:
        raise ValueError(f"patch networks: unsupported image batch [{B}, 1, {H}, {W}] or patch count {n}")
    return torch.empty(nbytes, device=dev, dtype=torch.uint8)


def _check_image(image: torch.Tensor, who: str):
    if not isinstance(image, torch.Tensor) or image.dim() != 4 or image.shape[1] != 1:
        raise ValueError(f"image must be a [B, 1, H, W] tensor, got {getattr(image, 'shape', type(image))}")
    B, _, H, W = image.shape
    if B < 1 or H < 1 or W < 1 or H > 8192 or W > 8192 or B * H * W > 1 << 22:
        raise ValueError(f"image {list(image.shape)}: 1 <= H, W <= 8192 and B * H * W <= 2^22")
    if not image.is_cuda:
        raise RuntimeError(f"{who}: expected an image tensor on the GPU; openglue_amd has no CPU path")


class PatchPyramid:
    """The image pyramid the patches are cut from: level 0 is the image, each further level the previous one blurred with
    [1 4 6 4 1] / 16 in both directions (reflect border) and resized bilinearly to half size; built while min(h, w) >= 32."""

    def __init__(self, image: torch.Tensor, workspace: Optional[torch.Tensor] = None):
        _check_image(image, "PatchPyramid")
        B, _, H, W = image.shape
        dev = image.device
        self.B, self.H, self.W = B, H, W
        self.sizes, per_image = pyramid_geometry(H, W)
        self.buffer = torch.empty(max(1, B * per_image), device=dev, dtype=torch.float32)
        img = image.detach().to(torch.float32).contiguous()
        ws = workspace if workspace is not None else _scratch(B, H, W, 0, dev)
        _lib.call("og_patch_pyramid", dev, B, H, W, img.data_ptr(), self.buffer.data_ptr(), ws.data_ptr(), _lib.STREAM)

    @property
    def levels(self) -> List[torch.Tensor]:
        """views [B, 1, h, w] of the levels"""
        out, o = [], 0
        for h, w in self.sizes:
            out.append(self.buffer[o:o + self.B * h * w].view(self.B, 1, h, w))
            o += self.B * h * w
        return out

    def extract(self, lafs: torch.Tensor, upright: bool = False, normalize: bool = False) -> torch.Tensor:
        """lafs [B, N, 2, 3] -> patches [B, N, 1, 32, 32]; normalize: (x - mean) / (std + 1e-6) per patch, as the nets do first"""
        lafs = _lib.gpu_tensor(lafs, "lafs", convert=True)
        if lafs.dim() != 4 or lafs.shape[0] != self.B or tuple(lafs.shape[2:]) != (2, 3):
            raise ValueError(f"lafs must be [{self.B}, N, 2, 3], got {list(lafs.shape)}")
        n = lafs.shape[1]
        patches = torch.empty(self.B, n, 1, PS, PS, device=lafs.device, dtype=torch.float32)
        _lib.call("og_patch_extract", lafs.device, self.B, self.H, self.W, n, self.buffer.data_ptr(), lafs.data_ptr(), int(bool(upright)),
                  int(bool(normalize)), patches.data_ptr(), _lib.STREAM)
        return patches


def extract_patches(image: torch.Tensor, lafs: torch.Tensor, upright: bool = False) -> torch.Tensor:
    """kornia's extract_patches_from_pyramid(image, lafs, PS=32): [B, N, 1, 32, 32].  upright=True cuts from [scale(A) I | c]."""
    return PatchPyramid(image).extract(lafs, upright=upright)


class _PatchNet(nn.Module):
    kind = ""

    def __init__(self):
        super().__init__()
        self.features = patchnet_features(self.kind)
        self._packed: Optional[torch.Tensor] = None
        self._packed_key = None

    # ---------------------------------------------------------------- packing (once per load_state_dict / device)
    def _pack_tensors(self):
        f = self.features
        ts = []
        for i in CONV_IDX:
            ts += [f[i].weight, f[i + 1].running_mean, f[i + 1].running_var]
        ts.append(f[19].weight)
        ts += [f[20].running_mean, f[20].running_var] if self.kind == "hardnet" else [f[19].bias]
        return ts

    def _pack(self, device: torch.device) -> torch.Tensor:
        ts = self._pack_tensors()
        key = (str(device),) + tuple((t.data_ptr(), t._version) for t in ts)
        if self._packed is not None and self._packed_key == key:
            return self._packed
        lib = _lib.load()
        host = [t.detach().to("cpu", torch.float32).contiguous() for t in ts]
        ptrs = (C.c_void_p * len(host))(*[h.data_ptr() for h in host])
        blob = torch.empty(lib.og_patchnet_packed_bytes(KINDS[self.kind]), dtype=torch.uint8)
        _lib.check(lib.og_patchnet_pack(KINDS[self.kind], float(self.features[1].eps), ptrs, blob.data_ptr()), "og_patchnet_pack")
        self._packed = blob.to(device)
        self._packed_key = key
        return self._packed

    def _patches(self, patches: torch.Tensor) -> torch.Tensor:
        if self.training:
            raise NotImplementedError(f"{type(self).__name__}: training-mode BatchNorm is not supported; call .eval()")
        if not isinstance(patches, torch.Tensor) or not patches.is_cuda:
            raise RuntimeError(f"{type(self).__name__}: expected patches on the GPU; openglue_amd has no CPU path")
        if patches.dim() not in (4, 5) or tuple(patches.shape[-3:]) != (1, PS, PS):
            raise ValueError(f"patches must be [N, 1, 32, 32] or [B, N, 1, 32, 32], got {list(patches.shape)}")
        return patches.detach().to(torch.float32).contiguous().view(-1, PS, PS)

    def run(self, patches: torch.Tensor, lafs: Optional[torch.Tensor] = None, normalize: bool = True, want_out: bool = True,
            workspace: Optional[torch.Tensor] = None) -> Optional[torch.Tensor]:
        """patches [N, 1, 32, 32] (or [B, N, 1, 32, 32], flattened) -> the net's output [N, 128 / 3 / 2]; AffNet / OriNet also update
        `lafs` ([N, 2, 3], contiguous fp32) in place.  normalize=False: the patches were normalised by the extraction."""
        x = self._patches(patches)
        n, dev = x.shape[0], x.device
        width = {"hardnet": 128, "affnet": 3, "orinet": 2}[self.kind]
        out = torch.empty(n, width, device=dev, dtype=torch.float32) if want_out else None
        if lafs is not None and (self.kind == "hardnet" or not lafs.is_cuda or lafs.dtype != torch.float32 or not lafs.is_contiguous()
                                 or lafs.numel() != 6 * n):
            raise ValueError(f"{type(self).__name__}: lafs must be a contiguous fp32 GPU tensor [{n}, 2, 3]")
        if n == 0:
            return out
        ws = workspace if workspace is not None else _scratch(0, 0, 0, n, dev)
        _lib.call("og_patchnet_forward", dev, KINDS[self.kind], n, x.data_ptr(), int(bool(normalize)), self._pack(dev).data_ptr(),
                  _lib.ptr(out), _lib.ptr(lafs), ws.data_ptr(), _lib.STREAM)
        return out

    @torch.no_grad()
    def forward(self, patches: torch.Tensor) -> torch.Tensor:
        return self.run(patches)


class HardNet(_PatchNet):
    """HardNet (https://arxiv.org/abs/1705.10872): patches [N, 1, 32, 32] -> unit descriptors [N, 128]"""
    kind = "hardnet"


class AffNet(_PatchNet):
    """AffNet (https://arxiv.org/abs/1711.06704) as kornia's LAFAffNetShapeEstimator(preserve_orientation=True): forward(patches)
    gives the three tanh outputs; estimate(lafs, pyramid) the reshaped LAFs."""
    kind = "affnet"

    @torch.no_grad()
    def estimate(self, lafs: torch.Tensor, pyramid: PatchPyramid, workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
        lafs = _lib.gpu_tensor(lafs, "lafs", convert=True).clone()
        self.run(pyramid.extract(lafs, upright=True, normalize=True), lafs, normalize=False, want_out=False, workspace=workspace)
        return lafs


class OriNet(_PatchNet):
    """OriNet: patches [N, 1, 32, 32] -> the two tanh outputs (y0, y1); the angle is atan2(y0 + 1e-8, y1 + 1e-8)"""
    kind = "orinet"


class LAFOrienter(nn.Module):
    """kornia's LAFOrienter(32, angle_detector=OriNet): A <- A rot(angle) with the angle from patches cut at the current LAF"""

    def __init__(self):
        super().__init__()
        self.angle_detector = OriNet()

    @torch.no_grad()
    def forward(self, lafs: torch.Tensor, pyramid: PatchPyramid, workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
        lafs = _lib.gpu_tensor(lafs, "lafs", convert=True).clone()
        self.angle_detector.run(pyramid.extract(lafs, normalize=True), lafs, normalize=False, want_out=False, workspace=workspace)
        return lafs


class DoGAffNetHardNet(nn.Module):
    """DoGAffNetHardNet(max_keypoints=-1, nms_diameter=9.): the reference's OPENCVDoGAffNetHardNet."""

    def __init__(self, max_keypoints: int = -1, nms_diameter: float = 9.):
        super().__init__()
        self.max_keypoints = max_keypoints
        self.nms_diameter = nms_diameter
        self.descriptor_dim = 128
        self.detector = SIFT(max_keypoints, nms_diameter)            # the DoG stage; its descriptor is not computed
        self.hardnet = HardNet()
        self.affnet = AffNet()
        self.orinet = LAFOrienter()
        self.eval()

    def detect(self, image: torch.Tensor):
        """the DoG stage -> lafs [B, N, 2, 3], responses [B, N] (one synchronisation: the counts)"""
        det = self.detector
        det.max_keypoints, det.nms_diameter = self.max_keypoints, self.nms_diameter
        det._check(image)
        B, _, H, W = image.shape
        dev, geom = image.device, sift_geometry(H, W)
        ws = det.workspace(B, H, W, dev)
        counts = det.new_counts(B, dev)
        gauss, dog = det.pyramid(image, ws)
        det_i, det_f = det.detect(dog, H, W, counts, ws)
        ori_i, ori_f = det.orient(gauss, H, W, det_i, det_f, counts, ws)
        sel = det.select(H, W, ori_i, ori_f, counts, ws)
        n = det.check_counts(counts.cpu(), B, geom)
        # og_sift_gather copies 128 descriptor floats per kept row next to the LAF; nothing was described, so it copies scratch
        # into a buffer that is dropped here
        desc = torch.empty(B, geom.cap2, 128, device=dev, dtype=torch.float32)
        lafs, scores, _ = det.gather(H, W, n, sel, ori_f, desc)
        return lafs, scores

    @torch.no_grad()
    def describe(self, image: torch.Tensor, lafs: torch.Tensor):
        """lafs [B, N, 2, 3] from the detector -> (final lafs, descriptors [B, N, 128]); no host synchronisation"""
        _check_image(image, "DoGAffNetHardNet")
        B, _, H, W = image.shape
        n = lafs.shape[1]
        dev = image.device
        if n == 0:
            return lafs, torch.empty(B, 0, 128, device=dev, dtype=torch.float32)
        ws = _scratch(B, H, W, B * n, dev)
        pyr = PatchPyramid(image, ws)
        lafs = self.affnet.estimate(lafs, pyr, ws)
        lafs = self.orinet(lafs, pyr, ws)
        desc = self.hardnet.run(pyr.extract(lafs, normalize=True), normalize=False, workspace=ws)
        return lafs, desc.view(B, n, 128)

    @torch.no_grad()
    def forward(self, image: torch.Tensor, mask=None):
        """image [B, 1, H, W] in [0, 1] -> lafs [B, N, 2, 3], scores [B, N] (DoG responses), descriptors [B, N, 128] (mask is ignored,
        as in the reference)"""
        lafs, scores = self.detect(image)
        lafs, desc = self.describe(image, lafs)
        return lafs, scores, desc


methods = {"DoGAffNetHardNet": DoGAffNetHardNet}
