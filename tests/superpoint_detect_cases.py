"""Crafted inputs for the stage-level tests of SuperPoint inference (csrc/superpoint.hip: sp_nms_kernel, sp_scan_kernel, sp_compact_kernel,
sp_select_kernel, sp_describe_kernel).  tests/test_superpoint_detect_cases_cpu.py proves on the CPU that every case reaches the edge it
names; tests/test_gpu_superpoint_stages.py feeds the same tensors to SuperPointNet.detect / .describe and asks for exact equality with the
float64 restatement (tests/superpoint_ref.py).

Given an fp32 heatmap the selection is a pure comparison of fp32 values, so none of this needs a tolerance.  Everything here is plain
numpy / torch on the CPU and deterministic: filler is a seeded permutation (pairwise distinct values), peaks are written by hand.

A case: name, heat [B, Hh, Wh] float32, k (nms_kernel), border, thr, max_kpts, edge (what it reaches, one line) and what the CPU test
asserts of it: kept / dropped (named pixels (b, y, x)), ties (groups of pixels whose values are bit-equal), n_cand (per image, None where
filler adds candidates of its own), m (the kept count, None likewise), order (per image "raster" / "desc").

The threshold: F.threshold on an fp32 tensor compares with the threshold cast to fp32 (ATen casts the scalar to the tensor's type), and so
does the kernel, which takes a C float.  thr32() is that value; the float64 restatement has to be given it, not the Python double
(0.1 rounds UP in fp32: a peak of value float32(0.1) is above the double 0.1 and not above the threshold that is applied).
"""
from types import SimpleNamespace

import numpy as np
import torch

SEG = 256                                            # SP_NMS_SEG of the source: columns per NMS workgroup
TILE = 256                                           # candidates per tile of sp_select_kernel


def thr32(thr):
    return float(np.float32(thr))


def up(v):
    return float(np.nextafter(np.float32(v), np.float32(np.inf)))


def down(v):
    return float(np.nextafter(np.float32(v), np.float32(-np.inf)))


def _filler(B, Hh, Wh, seed, lo, hi):
    """pairwise distinct values in (lo, hi): a seeded permutation of an even grid (spacing far above one fp32 ulp)"""
    n = B * Hh * Wh
    p = np.random.RandomState(seed).permutation(n).astype(np.float64)
    return (lo + (hi - lo) * (p + 1) / (n + 1)).astype(np.float32).reshape(B, Hh, Wh)


def _case(name, heat, k, border, thr, max_kpts, edge, kept=(), dropped=(), ties=(), n_cand=None, m=None, order=None):
    heat = torch.from_numpy(np.ascontiguousarray(heat, dtype=np.float32))
    assert heat.dim() == 3 and heat.shape[1] % 8 == 0 and heat.shape[2] % 8 == 0 and bool(torch.isfinite(heat).all())
    return SimpleNamespace(name=name, heat=heat, k=k, border=border, thr=thr, max_kpts=max_kpts, edge=edge, kept=list(kept),
                           dropped=list(dropped), ties=[list(t) for t in ties], n_cand=n_cand, m=m, order=order)


def _put(heat, pts, out, b, y, x, v):
    heat[b, y, x] = v
    out.append((b, y, x))
    pts.append((b, y, x))


# ---------------------------------------------------------------- seam
def seam_case(Wh, k):
    """Filler everywhere with thr = 0, so every local maximum of the filler is a candidate too and every halo column on both sides of
    every seam decides something.  Image 0: isolated peaks at x0 - 1, x0, x0 + 1 on rows 9 apart.  Image 1, per seam, with
    xr = min(x0 - 1 + r, Wh - 2) (the last column can never be kept, see edge_replicate): row 3 a pair at distance r, larger right of the
    seam; row 12 the same pair with the larger left of it; row 21 a pair at distance r + 1, both kept."""
    r = (k - 1) // 2
    heat = _filler(2, 32, Wh, 1000 + Wh + k, 0.01, 0.02)
    kept, dropped, pts = [], [], []
    for x0 in range(SEG, Wh, SEG):
        for i, y in enumerate((2, 11, 20)):
            _put(heat, pts, kept, 0, y, x0 - 1 + i, 0.6 + 0.05 * i)
        xr = min(x0 - 1 + r, Wh - 2)
        assert xr - r < x0 <= xr
        _put(heat, pts, dropped, 1, 3, xr - r, 0.5)
        _put(heat, pts, kept, 1, 3, xr, 0.7)
        _put(heat, pts, kept, 1, 12, xr - r, 0.75)
        _put(heat, pts, dropped, 1, 12, xr, 0.55)
        _put(heat, pts, kept, 1, 21, xr - r - 1, 0.52)
        _put(heat, pts, kept, 1, 21, xr, 0.72)
    return _case(f"seam-w{Wh}-k{k}", heat, k, 0, 0.0, -1, f"peaks and pairs across the 256-column seams of a {Wh}-wide row, radius {r}",
                 kept=kept, dropped=dropped)


# ---------------------------------------------------------------- plateau
def plateau_case(k):
    r = (k - 1) // 2
    assert r <= 4
    heat = _filler(1, 32, 64, 1100 + k, 0.01, 0.02)
    kept, dropped, pts = [], [], []
    _put(heat, pts, dropped, 0, 5, 5, 0.5)
    _put(heat, pts, dropped, 0, 5, 6, 0.5)
    _put(heat, pts, dropped, 0, 5, 20, 0.6)
    _put(heat, pts, dropped, 0, 5 + r, 20 + r, 0.6)                  # the corner of the window: Chebyshev distance exactly r
    _put(heat, pts, kept, 0, 5, 40, 0.7)
    _put(heat, pts, kept, 0, 5 + r + 1, 40 + r + 1, 0.7)
    block = []
    for y in range(20, 23):
        for x in range(8, 11):
            _put(heat, pts, block, 0, y, x, 0.8)
    return _case(f"plateau-k{k}", heat, k, 0, 0.005, -1, f"equal maxima: adjacent, at distance r = {r}, at r + 1, a 3 x 3 block",
                 kept=kept, dropped=dropped + block, ties=[pts[0:2], pts[2:4], pts[4:6], block])


# ---------------------------------------------------------------- edge_replicate
def edge_case(k):
    assert (k - 1) // 2 <= 4
    heat = _filler(1, 24, 40, 1200 + k, 0.01, 0.02)
    kept, dropped, pts = [], [], []
    for (y, x), v in zip([(0, 0), (23, 39), (0, 20), (23, 20), (16, 0), (16, 39)], (0.95, 0.9, 0.8, 0.81, 0.82, 0.83)):
        _put(heat, pts, dropped, 0, y, x, v)
    for (y, x), v in zip([(1, 10), (22, 10), (10, 1), (10, 38)], (0.7, 0.71, 0.72, 0.73)):
        _put(heat, pts, kept, 0, y, x, v)
    return _case(f"edge_replicate-k{k}", heat, k, 0, 0.005, -1, "border 0: the global maximum in a corner and maxima on all four edges are "
                 "dropped (replicate padding shows them a copy of themselves), peaks one pixel in are kept", kept=kept, dropped=dropped)


# ---------------------------------------------------------------- tiny
def tiny_cases():
    out = []
    a = _filler(1, 8, 8, 1300, 0.01, 0.02)
    a[0, 3, 4] = 0.9
    out.append(_case("tiny-8x8-k17", a, 17, 0, 0.005, -1, "radius 8 on an 8 x 8 image: every window is the whole image, only the global "
                     "maximum is kept", kept=[(0, 3, 4)], n_cand=[1], m=1, order=["raster"]))
    b = np.concatenate([a, _filler(1, 8, 8, 1301, 0.01, 0.02)])
    b[1, 0, 4] = 0.9
    out.append(_case("tiny-8x8-k17-pair", b, 17, 0, 0.005, -1, "the same beside an image whose global maximum sits on the top edge: "
                     "counts (1, 0), min_stack keeps 0", kept=[(0, 3, 4)], dropped=[(1, 0, 4)], n_cand=[1, 0], m=0, order=["desc", "desc"]))
    c = _filler(1, 8, 264, 1302, 0.01, 0.02)
    c[0, 3, 250], c[0, 4, 258], c[0, 2, 241] = 0.7, 0.6, 0.65
    out.append(_case("tiny-8x264-k17", c, 17, 0, 0.0, -1, "radius 8 on 8 rows: every row coordinate of the halo is clamped; a pair at "
                     "distance 8 across the seam, a third peak at distance 9", kept=[(0, 3, 250), (0, 2, 241)], dropped=[(0, 4, 258)]))
    return out


# ---------------------------------------------------------------- threshold
def threshold_cases():
    out = []
    for thr in (0.005, 0.1):
        t = thr32(thr)
        h = np.zeros((1, 16, 32), np.float32)
        h[0, 4, 4], h[0, 4, 10], h[0, 4, 16], h[0, 10, 4] = t, up(t), down(t), 0.5
        out.append(_case(f"threshold-{thr}", h, 3, 0, thr, -1, f"isolated peaks at float32({thr}), one ulp above and one ulp below",
                         kept=[(0, 4, 10), (0, 10, 4)], dropped=[(0, 4, 4), (0, 4, 16)], n_cand=[2], m=2, order=["raster"]))
    h = np.concatenate([_filler(1, 16, 32, 1400, -0.6, -0.5), np.full((1, 16, 32), -2.0, np.float32)])
    kept, dropped = [], []
    for b in (0, 1):
        h[b, 4, 4], h[b, 4, 10], h[b, 10, 4] = 0.0, -0.0, -0.25
        dropped += [(b, 4, 4), (b, 4, 10)]
        kept.append((b, 10, 4))
    h[0, 10, 12] = 0.3
    h[1, 10, 12], h[1, 10, 20], h[1, 10, 28] = -1.0, up(-1.0), down(-1.0)
    kept += [(0, 10, 12), (1, 10, 20)]
    dropped += [(1, 10, 12), (1, 10, 28)]
    out.append(_case("threshold-negative", h, 3, 0, -1.0, -1, "thr = -1: isolated 0.0 and -0.0 are above it and dropped by the != 0 rule, "
                     "-0.25 over a more negative background is kept; exactly -1 and its two neighbours in fp32",
                     kept=kept, dropped=dropped))
    return out


# ---------------------------------------------------------------- borders
def border_case(border, filler):
    Hh, Wh = 24, 40
    h = _filler(1, Hh, Wh, 1500 + border, 0.01, 0.02) if filler else np.zeros((1, Hh, Wh), np.float32)
    kept, dropped, pts = [], [], []
    xs = [(border - 1, dropped), (border, kept), (Wh - border - 1, kept), (Wh - border, dropped)]
    for i, (x, to) in enumerate(xs):
        _put(h, pts, to, 0, 8 + 2 * i, x, 0.5 + 0.01 * i)
    ys = [(border - 1, dropped), (border, kept), (Hh - border - 1, kept), (Hh - border, dropped)]
    for i, (y, to) in enumerate(ys):
        _put(h, pts, to, 0, y, 16 + 2 * i, 0.6 + 0.01 * i)
    return _case(f"borders-b{border}" + ("-filler" if filler else ""), h, 3, border, 0.0 if filler else 0.005, -1,
                 f"peaks at border - 1, border, size - border - 1, size - border in x and in y, border {border}", kept=kept, dropped=dropped,
                 n_cand=None if filler else [4], m=None if filler else 4, order=["raster"])


def border_all_cases():
    h = _filler(1, 16, 24, 1600, 0.01, 0.02)
    return [_case(f"borders-all-b{b}", h, 3, b, 0.0, -1, f"border {b} >= size / 2 of a 16 x 24 image: nothing is kept", n_cand=[0], m=0,
                  order=["raster"]) for b in (8, 12)]


# ---------------------------------------------------------------- lattice and what is built from it
def lattice_sites(Hh, Wh):
    """every (odd y, odd x) but the last row and column: with nms_kernel 3 over a zero background the densest set of candidates"""
    return [(y, x) for y in range(1, Hh - 1, 2) for x in range(1, Wh - 1, 2)]


def lattice_image(Hh, Wh, values):
    """the first len(values) lattice sites in raster order take `values`.  (Hh / 2 - 1) (Wh / 2 - 1) is 1 mod 4 for sizes that are
    multiples of 8, so no shape has exactly 256 or 512 sites: the counts are reached by leaving the tail of the lattice empty."""
    sites = lattice_sites(Hh, Wh)
    assert len(values) <= len(sites)
    h = np.zeros((Hh, Wh), np.float32)
    for (y, x), v in zip(sites, values):
        h[y, x] = v
    return h


def distinct_values(n, seed):
    p = np.random.RandomState(seed).permutation(n).astype(np.float64)
    return (0.1 + 0.8 * (p + 1) / (n + 1)).astype(np.float32)


LATTICE_SHAPES = [(16, 88, 256), (16, 88, 257), (24, 104, 512), (8, 776, 1161)]      # (Hh, Wh, candidates)


def lattice_cases():
    out = []
    for Hh, Wh, n in LATTICE_SHAPES:
        eq = lattice_image(Hh, Wh, np.full(n, 0.5, np.float32))[None]
        di = lattice_image(Hh, Wh, distinct_values(n, 1700 + n))[None]
        out.append(_case(f"lattice-equal-{n}", eq, 3, 0, 0.005, -1, f"{n} equal peaks, uncut", n_cand=[n], m=n, order=["raster"]))
        out.append(_case(f"lattice-distinct-{n}", di, 3, 0, 0.005, -1, f"{n} distinct peaks, uncut", n_cand=[n], m=n, order=["raster"]))
        out.append(_case(f"lattice-distinct-{n}-cut", di, 3, 0, 0.005, n - 1, f"{n} distinct peaks, the lowest cut off: ranks counted over "
                         f"{-(-n // TILE)} candidate tiles", n_cand=[n], m=n - 1, order=["desc"]))
    return out


def topk_cases():
    out = []
    Hh, Wh, n = 16, 88, 301
    eq = lattice_image(Hh, Wh, np.full(n, 0.5, np.float32))[None]
    for k in (1, 255, 256, 257, n - 1, n, n + 1, 0):
        cut = k < n
        out.append(_case(f"topk_ties-{n}-k{k}", eq, 3, 0, 0.005, k, f"{n} equal peaks, max_keypoints {k}: "
                         + ("the lowest raster indices in raster order" if cut else "the full raster list"), n_cand=[n],
                         m=k if cut else n, order=["desc" if cut else "raster"]))
    Hh, Wh, n = 24, 104, 561
    two = lattice_image(Hh, Wh, np.where(np.arange(n) % 2 == 0, 0.8, 0.4).astype(np.float32))[None]
    for k in (200, 481):
        out.append(_case(f"topk_ties-interleaved-k{k}", two, 3, 0, 0.005, k, "281 peaks of 0.8 interleaved with 280 of 0.4: the cut falls "
                         f"inside the run of {'0.8' if k < 281 else '0.4'}, whose kept part spans two candidate tiles", n_cand=[n], m=k,
                         order=["desc"]))
    return out


def min_stack_cases():
    Hh, Wh = 24, 104
    img = lambda n, seed: lattice_image(Hh, Wh, distinct_values(n, seed))
    out = []

    def add(name, counts, k, m, order, edge):
        heat = np.stack([img(n, 1800 + 10 * i + n) for i, n in enumerate(counts)])
        out.append(_case(f"min_stack-{name}", heat, 3, 0, 0.005, k, edge, n_cand=list(counts), m=m, order=order))

    add("empty-middle", (300, 0, 300), -1, 0, ["desc"] * 3, "counts (300, 0, 300): every image keeps 0")
    add("unequal", (300, 257, 500), -1, 257, ["desc"] * 3, "pairwise different counts: all keep 257 in descending order, the smallest included")
    add("mixed-order", (300, 500), 300, 300, ["raster", "desc"], "max_keypoints 300: image 0 uncut in raster order, image 1 cut, descending")
    add("equal", (300, 300), -1, 300, ["raster", "raster"], "equal counts, uncut: raster order in both")
    add("unequal-caps", (300, 500), 400, 300, ["desc", "desc"], "max_keypoints 400: c_b = (300, 400), both cut to 300 in descending order")
    return out


def all_cases():
    out = [seam_case(Wh, k) for Wh in (264, 512, 520) for k in (3, 9, 17)]
    out += [plateau_case(k) for k in (3, 9)] + [edge_case(k) for k in (3, 9)] + tiny_cases() + threshold_cases()
    out += [border_case(b, f) for b in (1, 4, 8) for f in (False, True)] + border_all_cases()
    out += lattice_cases() + topk_cases() + min_stack_cases()
    names = [c.name for c in out]
    assert len(set(names)) == len(names)
    return out


CASES = {c.name: c for c in all_cases()}


# ---------------------------------------------------------------- describe
DESCRIBE_SHAPES = [(1, 1), (1, 33), (2, 3), (4, 65)]                 # (Hc, Wc) of the coarse descriptor map
DESCRIBE_N = [1, 2, 3, 4, 5, 255, 257]                               # keypoints per call: sp_describe_kernel takes 4 per workgroup


def zero_cells(Hc, Wc):
    """rectangular blocks of cells that the zero variant clears (rectangles: a pixel on their rim keeps taps that share their one small
    weight factor, which F.normalize cancels, so no output is ill-conditioned)"""
    if (Hc, Wc) == (1, 1):
        return [(0, 0)]
    if Hc == 1:
        return [(0, 0), (0, Wc - 1)] + [(0, c) for c in range(10, 14)]
    if (Hc, Wc) == (2, 3):
        return [(0, 0), (0, 1), (1, 0), (1, 1)]
    return [(0, 0), (Hc - 1, Wc - 1)] + [(r, c) for r in (1, 2) for c in range(20, 24)]


def describe_maps(Hc, Wc, B, zero):
    """seeded unit-norm descriptors [B, Hc, Wc, 256] float32, different per image"""
    d = np.random.RandomState(1900 + 100 * Hc + Wc + B).standard_normal((B, Hc, Wc, 256))
    d = d / np.linalg.norm(d, axis=-1, keepdims=True)
    if zero:
        for r, c in zero_cells(Hc, Wc):
            d[:, r, c] = 0.0
    return torch.from_numpy(d.astype(np.float32))


def describe_pixels(Hc, Wc):
    """raster indices in a seeded order: every pixel of a small image; of a larger one all four corners, both pixels either side of every
    cell boundary along one row and one column, the last row, the last column and 64 others"""
    Hh, Wh = Hc * 8, Wc * 8
    rs = np.random.RandomState(2000 + 100 * Hc + Wc)
    if Hh * Wh <= 512:
        return rs.permutation(Hh * Wh).tolist()
    row, col = (3 if Hc == 1 else Hh // 2 + 1), 13
    pix = {(0, 0), (0, Wh - 1), (Hh - 1, 0), (Hh - 1, Wh - 1)}
    pix |= {(row, x) for c in range(1, Wc) for x in (8 * c - 1, 8 * c)} | {(y, col) for c in range(1, Hc) for y in (8 * c - 1, 8 * c)}
    pix |= {(Hh - 1, x) for x in range(Wh)} | {(y, Wh - 1) for y in range(Hh)}
    pix |= {(int(i) // Wh, int(i) % Wh) for i in rs.choice(Hh * Wh, 64, replace=False)}
    idx = np.array(sorted(y * Wh + x for y, x in pix))
    return idx[rs.permutation(len(idx))].tolist()


def describe_runs(Hc, Wc):
    """the (n, first) runs of one shape: run n takes pixels[first : first + n] cyclically, so that the runs of DESCRIBE_N walk through
    the list, and one last run holds all of it when the list is longer than they reach"""
    total, runs, first = len(describe_pixels(Hc, Wc)), [], 0
    for n in DESCRIBE_N:
        runs.append((n, first % total))
        first += n
    if first < total:
        runs.append((total, 0))
    return runs


def take(pixels, first, n, shift=0):
    return [pixels[(first + shift + i) % len(pixels)] for i in range(n)]


def taps(Hc, Wc, idx):
    """float64 sample position of sample_desc_from_points + grid_sample (align_corners=False) for raster indices idx: ix, iy and the
    corner cell x0, y0 of the four taps (x0 + 1, y0 + 1 are the others)"""
    Hh, Wh = Hc * 8, Wc * 8
    idx = np.asarray(idx, np.int64)
    x, y = (idx % Wh).astype(np.float64), (idx // Wh).astype(np.float64)
    ix = ((x - 3.5) / (Wh - 4.5) * 2 * Wc - 1) / 2
    iy = ((y - 3.5) / (Hh - 4.5) * 2 * Hc - 1) / 2
    return ix, iy, np.floor(ix).astype(np.int64), np.floor(iy).astype(np.int64)


def tap_stats(Hc, Wc, idx):
    """how many of the pixels have a tap outside the coarse map on each side and in each corner, and how many have all four inside"""
    _, _, x0, y0 = taps(Hc, Wc, idx)
    left, right, top, bottom = x0 < 0, x0 + 1 >= Wc, y0 < 0, y0 + 1 >= Hc
    return {"left": int(left.sum()), "right": int(right.sum()), "top": int(top.sum()), "bottom": int(bottom.sum()),
            "top-left": int((top & left).sum()), "top-right": int((top & right).sum()), "bottom-left": int((bottom & left).sum()),
            "bottom-right": int((bottom & right).sum()), "inside": int((~(left | right | top | bottom)).sum())}


def all_taps_zero(Hc, Wc, idx, zero=True):
    """per pixel: every tap is outside the map or (zero variant) on a cleared cell, so the descriptor is exactly the zero vector"""
    _, _, x0, y0 = taps(Hc, Wc, idx)
    cleared = set(zero_cells(Hc, Wc)) if zero else set()
    out = []
    for a, b in zip(x0.tolist(), y0.tolist()):
        cells = [(b + dy, a + dx) for dy in (0, 1) for dx in (0, 1)]
        out.append(all(not (0 <= r < Hc and 0 <= c < Wc) or (r, c) in cleared for r, c in cells))
    return np.array(out)
