"""Float64 restatement of SuperPoint inference in torch on the CPU (reference models/features/superpoint/model.py, utils.py,
models/features/utils.py min_stack, kornia nms2d), with the margin of every discrete decision.

dense()   -> heatmap [B, Hc*8, Wc*8] (pre-NMS) and coarse descriptors [B, Hc, Wc, D] (NHWC, unit norm)
select()  -> per image: raster indices and scores in output order, and the decision margins:
             pixel margin  = how far the keep / drop decision of a pixel is from flipping (NMS: x - max of the k*k-1
                             neighbours, threshold: x - thr; the border rule is exact), +inf where a test fails clearly
             cut margin    = |score - the score at the top-k / min_stack cut| for candidates of an image that was cut
describe() -> sample_desc_from_points at given (x, y) in float64.
A position is EXEMPT when its margin is below eps.
"""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F

CONVS = [f"conv{i}{s}" for i in range(1, 5) for s in "ab"]


def _bn(sd, name, x):
    if f"{name}.weight" not in sd:
        return x
    g, b, m, v = (sd[f"{name}.{k}"].to(x.dtype) for k in ("weight", "bias", "running_mean", "running_var"))
    s = (g / torch.sqrt(v + 1e-5)).view(1, -1, 1, 1)
    return (x - m.view(1, -1, 1, 1)) * s + b.view(1, -1, 1, 1)


def _conv(sd, name, x):
    w, b = sd[f"{name}.weight"].to(x.dtype), sd[f"{name}.bias"].to(x.dtype)
    return F.conv2d(x, w, b, padding=w.shape[-1] // 2)


def dense(sd, image: torch.Tensor, dtype=torch.float64):
    bn = "bn1a.weight" in sd
    x = image.to(dtype)
    for i, name in enumerate(CONVS):
        x = F.relu(_bn(sd, "bn" + name[4:], _conv(sd, name, x)) if bn else _conv(sd, name, x))
        if name.endswith("b") and i < 6:
            x = F.max_pool2d(x, 2, 2)
    pa = F.relu(_bn(sd, "bnPa", _conv(sd, "convPa", x)) if bn else _conv(sd, "convPa", x))
    logits = _bn(sd, "bnPb", _conv(sd, "convPb", pa)) if bn else _conv(sd, "convPb", pa)
    da = F.relu(_bn(sd, "bnDa", _conv(sd, "convDa", x)) if bn else _conv(sd, "convDa", x))
    d = _bn(sd, "bnDb", _conv(sd, "convDb", da)) if bn else _conv(sd, "convDb", da)
    d = d / torch.norm(d, p=2, dim=1, keepdim=True)
    s = F.softmax(logits, 1)[:, :-1]
    b, _, h, w = s.shape
    heat = s.permute(0, 2, 3, 1).reshape(b, h, w, 8, 8).permute(0, 1, 3, 2, 4).reshape(b, h * 8, w * 8)
    return heat, d.permute(0, 2, 3, 1).contiguous()


def max_neighbours(heat: torch.Tensor, k: int) -> torch.Tensor:
    """Maximum over the k*k-1 neighbours (centre excluded) under replicate padding, [B, H, W]."""
    r = (k - 1) // 2
    H, W = heat.shape[-2:]
    p = F.pad(heat[:, None], (r, r, r, r), mode="replicate")[:, 0]
    out = torch.full_like(heat, -math.inf)
    for dy in range(k):
        for dx in range(k):
            if dy != r or dx != r:
                out = torch.maximum(out, p[:, dy:dy + H, dx:dx + W])
    return out


def pixel_decisions(heat: torch.Tensor, k: int, border: int, thr: float):
    """-> keep [B, H, W] bool, margin [B, H, W] (inf where the decision is not near a flip)."""
    B, H, W = heat.shape
    m_nms = heat - max_neighbours(heat, k)
    m_thr = heat - thr
    yy = torch.arange(H).view(1, H, 1)
    xx = torch.arange(W).view(1, 1, W)
    inb = (xx >= border) & (xx < W - border) & (yy >= border) & (yy < H - border)
    inb = inb.expand(B, H, W)
    keep = (m_nms > 0) & (m_thr > 0) & (heat != 0) & inb
    zero = torch.zeros_like(heat)
    drop_m = torch.maximum(torch.where(m_nms <= 0, -m_nms, zero), torch.where(m_thr <= 0, -m_thr, zero))   # the clearest failure decides
    margin = torch.where(keep, torch.minimum(m_nms, m_thr), drop_m)
    margin = torch.where(inb, margin, torch.full_like(heat, math.inf))
    return keep, margin



def select(heat: torch.Tensor, k: int, border: int, thr: float, max_kpts: int):
    """-> list over images of dict(idx (raster, output order), score, margin_pix [H*W], cut_margin [n_cand] or None, order)."""
    B, H, W = heat.shape
    keep, margin = pixel_decisions(heat, k, border, thr)
    cands = []
    for b in range(B):
        idx = torch.nonzero(keep[b].flatten()).flatten()
        cands.append((idx, heat[b].flatten()[idx]))
    cb = [len(i) if (max_kpts < 0 or max_kpts >= len(i)) else max_kpts for i, _ in cands]
    equal = all(c == cb[0] for c in cb)
    out = []
    for b, (idx, sc) in enumerate(cands):
        m = cb[b] if equal else min(cb)
        if equal and m == len(idx):
            out.append(dict(idx=idx, score=sc, margin_pix=margin[b].flatten(), cut_margin=None, order="raster", n_cand=len(idx)))
            continue
        # descending score, equal scores by raster index (idx is ascending, sort is stable)
        o = torch.sort(sc, descending=True, stable=True).indices
        kth = sc[o[m - 1]] if m > 0 else math.inf
        out.append(dict(idx=idx[o[:m]], score=sc[o[:m]], margin_pix=margin[b].flatten(), cut_margin=(sc - kth).abs(),
                        cand_idx=idx, order="desc", n_cand=len(idx)))
    return out


def describe(desc_nhwc: torch.Tensor, xy: torch.Tensor) -> torch.Tensor:
    """sample_desc_from_points for one image: desc [Hc, Wc, D], xy [N, 2] -> [N, D] (float64)."""
    Hc, Wc, D = desc_nhwc.shape
    H, W = Hc * 8, Wc * 8
    p = xy.to(torch.float64) - 4 + 0.5
    p = p / torch.tensor([W - 4.5, H - 4.5], dtype=torch.float64)
    p = p * 2 - 1
    d = F.grid_sample(desc_nhwc.permute(2, 0, 1)[None].to(torch.float64), p.view(1, 1, -1, 2), mode="bilinear", align_corners=False)
    d = d.view(D, -1).t()
    return F.normalize(d, p=2, dim=1)
