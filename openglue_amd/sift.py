"""SIFT keypoints and descriptors on HIP kernels: a drop-in for the reference's `sift_create_torch(max_keypoints, nms_diameter,
rootsift)` (models/features/opencv/_features.py: cv2.SIFT_create(contrastThreshold=-10000, edgeThreshold=-10000) behind
OpenCVFeatures and the torch wrapper), inference only.

`forward(image [B, 1, H, W], mask=None)` returns (lafs [B, N, 2, 3], scores [B, N], descriptors [B, N, 128]) on the GPU -- what
features.prepare_features_output and SuperGlue.match take.  Every step runs in csrc/sift.hip (og_sift_pyramid / _detect / _orient /
_describe / _select / _gather): no ATen, MIOpen, OpenCV, SciPy or kornia on the path, and no CPU path.

The detector and descriptor are Lowe 2004 with OpenCV's constants; tests/sift_ref.py is their float64 specification and DESIGN.md
section 4.11 lists where they knowingly differ from OpenCV (no bit parity with cv2.SIFT_create is claimed).  The code around them is
the reference's own (base.py): greedy radius NMS in descending response, the `max_keypoints` strongest, LAFs with mr_size 6 and
RootSIFT / L2 descriptor normalisation.  Output order is descending response; equal responses are ordered by (octave, layer, row,
column, orientation rank).  Because the NMS removes everything within the radius, distance 0 included, it keeps ONE orientation per
location, the strongest histogram peak; with nms_diameter <= 0 every peak >= 0.8 max is a keypoint of its own.  For B > 1 (which
the reference does not support) every image is cut to the batch-minimum count by top response (min_stack, as superpoint.py); no
keypoints give empty outputs.

One device -> host synchronisation per call: the counts, which size the outputs.
"""
from __future__ import annotations

import ctypes as C
from typing import List, NamedTuple, Tuple

import torch
import torch.nn as nn

from . import _lib

DESCRIPTOR_DIM = 128
MIN_HW, MAX_HW, MAX_PIXELS = 8, 8192, 1 << 22


class Geometry(NamedTuple):
    octaves: List[Tuple[int, int]]     # (h, w) of every octave built
    cap: int                           # keypoints per image
    cap2: int                          # oriented keypoints per image

    @property
    def gauss_floats(self) -> int:
        return sum(6 * h * w for h, w in self.octaves)

    @property
    def dog_floats(self) -> int:
        return sum(5 * h * w for h, w in self.octaves)


def geometry(H: int, W: int) -> Geometry:
    out = (C.c_int32 * 35)()
    _lib.check(_lib.load().og_sift_geometry(H, W, out), "og_sift_geometry")
    return Geometry([(out[3 + 2 * o], out[4 + 2 * o]) for o in range(out[0])], out[1], out[2])


def split_octaves(flat: torch.Tensor, geom: Geometry, levels: int) -> List[torch.Tensor]:
    """gauss (levels = 6) or dog (levels = 5) buffer [B, floats] -> per octave views [B, levels, h, w]"""
    out, o = [], 0
    for h, w in geom.octaves:
        out.append(flat[:, o:o + levels * h * w].view(flat.shape[0], levels, h, w))
        o += levels * h * w
    return out


class SIFT(nn.Module):
    """SIFT(max_keypoints=-1, nms_diameter=9., rootsift=True): the reference's sift_create_torch.  upright=True skips the orientation
    histogram (angle 0); quantize=False keeps the descriptor in float instead of OpenCV's bytes (min(255, round(512 v)))."""

    def __init__(self, max_keypoints: int = -1, nms_diameter: float = 9., rootsift: bool = True, upright: bool = False,
                 quantize: bool = True):
        super().__init__()
        self.max_keypoints = max_keypoints
        self.nms_diameter = nms_diameter
        self.rootsift = rootsift
        self.upright = upright
        self.quantize = quantize
        self.descriptor_dim = DESCRIPTOR_DIM

    # ---------------------------------------------------------------- checks
    def _check_args(self):
        if isinstance(self.max_keypoints, bool) or not isinstance(self.max_keypoints, int):
            raise ValueError(f"max_keypoints must be an int, got {self.max_keypoints!r}")
        d = float(self.nms_diameter)
        if d != d or d in (float("inf"), float("-inf")):
            raise ValueError(f"nms_diameter must be finite, got {self.nms_diameter!r}")

    def _check(self, image: torch.Tensor):
        self._check_args()
        if not isinstance(image, torch.Tensor) or image.dim() != 4 or image.shape[1] != 1:
            raise ValueError(f"image must be a [B, 1, H, W] tensor, got {getattr(image, 'shape', type(image))}")
        B, _, H, W = image.shape
        if B < 1 or not (MIN_HW <= H <= MAX_HW and MIN_HW <= W <= MAX_HW) or B * H * W > MAX_PIXELS:
            raise ValueError(f"image {list(image.shape)}: {MIN_HW} <= H, W <= {MAX_HW} and B * H * W <= 2^22")
        if not image.is_cuda:
            raise RuntimeError("SIFT: expected an image tensor on the GPU; openglue_amd has no CPU path")

    def workspace(self, B: int, H: int, W: int, dev) -> torch.Tensor:
        n = _lib.load().og_sift_workspace_bytes(B, H, W)
        if n == 0:
            raise ValueError(f"SIFT: unsupported image batch [{B}, 1, {H}, {W}]")
        return torch.empty(n, device=dev, dtype=torch.uint8)

    @staticmethod
    def new_counts(B: int, dev) -> torch.Tensor:
        return torch.zeros(4 * B + 1, device=dev, dtype=torch.int32)

    @staticmethod
    def check_counts(counts: torch.Tensor, B: int, geom: Geometry) -> int:
        """counts on the host -> rows every image puts out; raises where a stage ran out of room"""
        c = counts.tolist()
        for b in range(B):
            for what, v, cap in (("keypoints", c[b], geom.cap), ("oriented keypoints", c[B + b], geom.cap2),
                                 ("NMS neighbour entries", c[3 * B + b], 32 * geom.cap2)):
                if v < 0 or v > cap:
                    raise RuntimeError(f"SIFT: image {b} has {v} {what}, the buffers sized from the image hold {cap}")
        return c[4 * B]

    # ---------------------------------------------------------------- stages
    def pyramid(self, image: torch.Tensor, workspace: torch.Tensor):
        """-> gauss [B, gauss_floats], dog [B, dog_floats] (fp32; split_octaves gives the per-octave views)"""
        self._check(image)
        B, _, H, W = image.shape
        dev, geom = image.device, geometry(H, W)
        img = image.detach().to(torch.float32).contiguous()
        gauss = torch.empty(B, geom.gauss_floats, device=dev, dtype=torch.float32)
        dog = torch.empty(B, geom.dog_floats, device=dev, dtype=torch.float32)
        _lib.call("og_sift_pyramid", dev, B, H, W, img.data_ptr(), gauss.data_ptr(), dog.data_ptr(), workspace.data_ptr(), _lib.STREAM)
        return gauss, dog

    def detect(self, dog: torch.Tensor, H: int, W: int, counts: torch.Tensor, workspace: torch.Tensor):
        """-> det_i [B, cap, 4] int32 (octave, layer, row, column), det_f [B, cap, 4] float64 (x, y, size, response); counts[b] rows are valid"""
        B, dev, geom = dog.shape[0], dog.device, geometry(H, W)
        det_i = torch.zeros(B, geom.cap, 4, device=dev, dtype=torch.int32)
        det_f = torch.zeros(B, geom.cap, 4, device=dev, dtype=torch.float64)
        _lib.call("og_sift_detect", dev, B, H, W, dog.data_ptr(), det_i.data_ptr(), det_f.data_ptr(), counts.data_ptr(), workspace.data_ptr(),
                  _lib.STREAM)
        return det_i, det_f

    def orient(self, gauss: torch.Tensor, H: int, W: int, det_i: torch.Tensor, det_f: torch.Tensor, counts: torch.Tensor,
               workspace: torch.Tensor):
        """-> ori_i [B, cap2, 6] int32 (octave, layer, row, column, orientation rank, source keypoint), ori_f [B, cap2, 5] float32
        (x, y, size, angle, response); counts[B + b] rows are valid"""
        B, dev, geom = gauss.shape[0], gauss.device, geometry(H, W)
        ori_i = torch.zeros(B, geom.cap2, 6, device=dev, dtype=torch.int32)
        ori_f = torch.zeros(B, geom.cap2, 5, device=dev, dtype=torch.float32)
        _lib.call("og_sift_orient", dev, B, H, W, int(bool(self.upright)), gauss.data_ptr(), det_i.data_ptr(), det_f.data_ptr(),
                  counts.data_ptr(), ori_i.data_ptr(), ori_f.data_ptr(), workspace.data_ptr(), _lib.STREAM)
        return ori_i, ori_f

    def describe(self, gauss: torch.Tensor, H: int, W: int, ori_i: torch.Tensor, ori_f: torch.Tensor, counts: torch.Tensor,
                 normalize: bool = True):
        """-> desc [B, cap2, 128] float32, normalised (normalize=False: before the RootSIFT / L2 step, OpenCV's values); counts[B + b]
        rows are valid"""
        B, dev, geom = gauss.shape[0], gauss.device, geometry(H, W)
        desc = torch.empty(B, geom.cap2, DESCRIPTOR_DIM, device=dev, dtype=torch.float32)
        _lib.call("og_sift_describe", dev, B, H, W, int(bool(self.quantize)), int(bool(self.rootsift)) if normalize else -1,
                  gauss.data_ptr(), ori_i.data_ptr(),
                  ori_f.data_ptr(), counts.data_ptr(), desc.data_ptr(), _lib.STREAM)
        return desc

    def select(self, H: int, W: int, ori_i: torch.Tensor, ori_f: torch.Tensor, counts: torch.Tensor, workspace: torch.Tensor):
        """-> sel [B, cap2] int32: rows of ori_* in output order; counts[2B + b] kept per image, counts[4B] rows every image puts out"""
        self._check_args()
        B, dev, geom = ori_f.shape[0], ori_f.device, geometry(H, W)
        sel = torch.zeros(B, geom.cap2, device=dev, dtype=torch.int32)
        _lib.call("og_sift_select", dev, B, H, W, float(self.nms_diameter), int(self.max_keypoints), ori_i.data_ptr(), ori_f.data_ptr(),
                  counts.data_ptr(), sel.data_ptr(), workspace.data_ptr(), _lib.STREAM)
        return sel

    def gather(self, H: int, W: int, n: int, sel: torch.Tensor, ori_f: torch.Tensor, desc: torch.Tensor):
        B, dev = ori_f.shape[0], ori_f.device
        lafs = torch.empty(B, n, 2, 3, device=dev, dtype=torch.float32)
        scores = torch.empty(B, n, device=dev, dtype=torch.float32)
        descriptors = torch.empty(B, n, DESCRIPTOR_DIM, device=dev, dtype=torch.float32)
        _lib.call("og_sift_gather", dev, B, H, W, n, sel.data_ptr(), ori_f.data_ptr(), desc.data_ptr(), lafs.data_ptr(), scores.data_ptr(),
                  descriptors.data_ptr(), _lib.STREAM)
        return lafs, scores, descriptors

    @torch.no_grad()
    def forward(self, image: torch.Tensor, mask=None):
        """image [B, 1, H, W] in [0, 1] -> lafs [B, N, 2, 3], scores [B, N], descriptors [B, N, 128] (mask is ignored, as in the reference)."""
        self._check(image)
        B, _, H, W = image.shape
        dev, geom = image.device, geometry(H, W)
        ws = self.workspace(B, H, W, dev)
        counts = self.new_counts(B, dev)
        gauss, dog = self.pyramid(image, ws)
        det_i, det_f = self.detect(dog, H, W, counts, ws)
        ori_i, ori_f = self.orient(gauss, H, W, det_i, det_f, counts, ws)
        desc = self.describe(gauss, H, W, ori_i, ori_f, counts)
        sel = self.select(H, W, ori_i, ori_f, counts, ws)
        n = self.check_counts(counts.cpu(), B, geom)          # the one synchronisation
        return self.gather(H, W, n, sel, ori_f, desc)


def sift_create_torch(max_keypoints: int = -1, nms_diameter: float = 9., rootsift: bool = True) -> SIFT:
    return SIFT(max_keypoints, nms_diameter, rootsift)
