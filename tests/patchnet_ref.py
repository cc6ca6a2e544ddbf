"""The specification of openglue_amd/affnet_hardnet.py (csrc/patchnet.hip) restated in torch: pyramid, patch extraction, the three
patch networks and the LAF algebra of the reference's OPENCVDoGAffNetHardNet after its detector, a kornia 0.6-era reading.  Every
function computes in the dtype of its input: float64 is the specification, the same code in float32 gives the error a plain fp32
implementation makes (e32), from which the GPU tests take their tolerances.

Notation: a LAF is [A | c], scale(A) = sqrt |det A|, ori(A) = atan2(A01, A00), rot(t) = [[cos t, sin t], [-sin t, cos t]], PS = 32.
"""
import math

import torch
import torch.nn.functional as F

PS = 32
CONV_IDX = (0, 3, 6, 9, 12, 15)
STRIDES = (1, 1, 2, 1, 2, 1)
BN_EPS = 1e-5


# ---------------------------------------------------------------- pyramid
def pyramid(image):
    """image [B, 1, H, W] -> levels [B, 1, h_l, w_l]: blur [1 4 6 4 1] / 16 in both directions (reflect), bilinear resize to
    (floor(h / 2), floor(w / 2)), align_corners=False; built while min(h, w) >= PS"""
    k = torch.tensor([1.0, 4.0, 6.0, 4.0, 1.0], dtype=image.dtype) / 16.0
    levels, cur = [], image
    while min(cur.shape[-2:]) >= PS:
        levels.append(cur)
        h, w = cur.shape[-2:]
        x = F.pad(cur, (2, 2, 2, 2), mode="reflect")
        x = F.conv2d(F.conv2d(x, k.view(1, 1, 1, 5)), k.view(1, 1, 5, 1))
        cur = F.interpolate(x, size=(h // 2, w // 2), mode="bilinear", align_corners=False)
    return levels


# ---------------------------------------------------------------- LAF algebra
def scale_of(lafs):
    A = lafs[..., :2]
    return (A[..., 0, 0] * A[..., 1, 1] - A[..., 0, 1] * A[..., 1, 0]).abs().sqrt()


def rot(phi):
    c, s = torch.cos(phi), torch.sin(phi)
    return torch.stack([torch.stack([c, s], -1), torch.stack([-s, c], -1)], -2)


def upright_of(lafs):
    out = torch.zeros_like(lafs)
    s = scale_of(lafs)
    out[..., 0, 0] = s
    out[..., 1, 1] = s
    out[..., 2] = lafs[..., 2]
    return out


def level_of(lafs):
    """-> level max(0, floor(log2(2 scale / PS))) and its margin |log2(2 scale / PS) - nearest integer| (+inf below level 0's lower
    edge, where no rounding changes the level)"""
    t = torch.log2(2.0 * scale_of(lafs.double()) / PS)
    level = torch.clamp(torch.floor(t), min=0).long()
    margin = (t - torch.round(t)).abs()
    margin = torch.where(t < 0, torch.full_like(margin, math.inf), margin)
    return level, margin


# ---------------------------------------------------------------- patches
def sample_positions(laf, size0, size_l):
    """one LAF [2, 3] at level 0 -> pixel-index positions [PS, PS, 2] (x, y) in a level of size_l = (h, w)"""
    (h0, w0), (hl, wl) = size0, size_l
    A = laf[:, :2] * ((min(hl, wl) - 1) / (min(h0, w0) - 1))
    c = torch.stack([laf[0, 2] * (wl - 1) / (w0 - 1), laf[1, 2] * (hl - 1) / (h0 - 1)])
    g = (2.0 * torch.arange(PS, dtype=laf.dtype) + 1.0) / PS - 1.0
    gy, gx = torch.meshgrid(g, g, indexing="ij")                     # patch pixel (i, j): (g_j, g_i)
    grid = torch.stack([gx, gy], -1)                                 # [PS, PS, 2]
    return grid @ A.T + c - 0.5


def extract(levels, lafs, upright=False):
    """extract_patches_from_pyramid: lafs [B, N, 2, 3] -> patches [B, N, 1, PS, PS] in the dtype of the levels"""
    dtype = levels[0].dtype if levels else lafs.dtype
    lafs = lafs.to(dtype)
    B, N = lafs.shape[:2]
    level, _ = level_of(lafs)
    src = upright_of(lafs) if upright else lafs
    out = torch.zeros(B, N, 1, PS, PS, dtype=dtype)
    if not levels:
        return out
    size0 = tuple(levels[0].shape[-2:])
    for b in range(B):
        for i in range(N):
            L = int(level[b, i])
            if L >= len(levels):
                continue                                             # the level was not built: zeros
            hl, wl = levels[L].shape[-2:]
            p = sample_positions(src[b, i], size0, (hl, wl))
            grid = torch.stack([(2.0 * p[..., 0] + 1.0) / wl - 1.0, (2.0 * p[..., 1] + 1.0) / hl - 1.0], -1)
            out[b, i] = F.grid_sample(levels[L][b:b + 1], grid[None], mode="bilinear", padding_mode="border", align_corners=False)[0]
    return out


def normalize_patches(x):
    """(x - mean) / (std + 1e-6) per patch, unbiased std over the PS * PS pixels"""
    flat = x.flatten(-2)
    mean = flat.mean(-1)[..., None, None]
    std = flat.std(-1, unbiased=True)[..., None, None]
    return (x - mean) / (std + 1e-6)


# ---------------------------------------------------------------- networks
def net_forward(sd, kind, patches, prefix="features."):
    """patches [n, 1, PS, PS] -> HardNet [n, 128] unit descriptors, AffNet [n, 3], OriNet [n, 2] tanh outputs"""
    dt = patches.dtype
    P = lambda name: sd[prefix + name].to(dt)
    x = normalize_patches(patches)
    for i, stride in zip(CONV_IDX, STRIDES):
        x = F.conv2d(x, P(f"{i}.weight"), stride=stride, padding=1)
        x = (x - P(f"{i + 1}.running_mean").view(1, -1, 1, 1)) / torch.sqrt(P(f"{i + 1}.running_var").view(1, -1, 1, 1) + BN_EPS)
        x = F.relu(x)
    if kind == "hardnet":
        x = F.conv2d(x, P("19.weight"))
        x = (x - P("20.running_mean").view(1, -1, 1, 1)) / torch.sqrt(P("20.running_var").view(1, -1, 1, 1) + BN_EPS)
        x = x.flatten(1)
        return x / x.norm(dim=1, keepdim=True).clamp(min=1e-12)
    x = F.conv2d(x, P("19.weight"), P("19.bias"))
    return torch.tanh(x).flatten(1)


def affnet_update(lafs, xy):
    """LAFAffNetShapeEstimator(preserve_orientation=True): lafs [n, 2, 3], net outputs [n, 3]"""
    A = lafs[..., :2]
    one, zero = torch.ones_like(xy[:, 0]), torch.zeros_like(xy[:, 0])
    Ap = torch.stack([torch.stack([one + xy[:, 0], zero], -1), torch.stack([xy[:, 1], one + xy[:, 2]], -1)], -2)
    det = Ap[:, 0, 0] * Ap[:, 1, 1]
    unit = Ap / det.sqrt()[:, None, None]
    newA = scale_of(lafs)[:, None, None] * (unit @ rot(torch.atan2(A[:, 0, 1], A[:, 0, 0])))
    return torch.cat([newA, lafs[..., 2:]], -1)


def orinet_update(lafs, y):
    """LAFOrienter: A <- A rot(atan2(y0 + 1e-8, y1 + 1e-8))"""
    delta = torch.atan2(y[:, 0] + 1e-8, y[:, 1] + 1e-8)
    return torch.cat([lafs[..., :2] @ rot(delta), lafs[..., 2:]], -1)


def chain(image, lafs, sds):
    """image [B, 1, H, W], detector lafs [B, N, 2, 3], sds = {kind: state dict} -> final lafs [B, N, 2, 3], descriptors [B, N, 128]
    and the smallest level margin of each keypoint over the three extractions [B, N]"""
    dt = image.dtype
    lafs = lafs.to(dt)
    B, N = lafs.shape[:2]
    levels = pyramid(image)
    _, m0 = level_of(lafs)
    x = net_forward(sds["affnet"], "affnet", extract(levels, lafs, upright=True).flatten(0, 1))
    lafs = affnet_update(lafs.flatten(0, 1), x).view(B, N, 2, 3)
    _, m1 = level_of(lafs)
    y = net_forward(sds["orinet"], "orinet", extract(levels, lafs).flatten(0, 1))
    lafs = orinet_update(lafs.flatten(0, 1), y).view(B, N, 2, 3)
    _, m2 = level_of(lafs)
    desc = net_forward(sds["hardnet"], "hardnet", extract(levels, lafs).flatten(0, 1)).view(B, N, 128)
    return lafs, desc, torch.minimum(torch.minimum(m0, m1), m2)
