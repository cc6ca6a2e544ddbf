"""Float64 restatement of the SIFT extractor (openglue_amd/sift.py, csrc/sift.hip): Lowe 2004 with OpenCV's constants, stage by stage
from given inputs.  NumPy only.  It is the specification the GPU is tested against; it is not OpenCV and claims no bit parity with it.

    quantize -> pyramid (base image, Gaussian octaves, DoG) -> detect (extrema + fp64 refinement) -> orient -> describe -> select -> lafs

Keypoints travel the way the kernels pass them: `ki` int [n, 4] = (octave, layer, row, column) of the converged sample, and the
fields of a cv2.KeyPoint (x, y, size, angle, response).  detect returns them in float64; orient rounds them to float32 (a
cv2.KeyPoint holds floats), and describe / select take those float32 values.
"""
import math

import numpy as np

S = 3                     # nOctaveLayers
SIGMA = 1.6
BORDER = 5                # SIFT_IMG_BORDER
MAX_STEPS = 5             # SIFT_MAX_INTERP_STEPS
ORI_BINS = 36
D, NB = 4, 8              # descriptor: D x D spatial bins, NB orientation bins
MIN_SIDE = 2 * BORDER + 1


def _round(x):
    """round half up, the rounding of every discrete decision here (and in the kernels)"""
    return np.floor(np.asarray(x, dtype=np.float64) + 0.5)


def quantize(image):
    """image in [0, 1] (any float dtype) -> the 8-bit values as float64: trunc(255.f * x) with an fp32 multiply, clamped."""
    x = np.asarray(image, dtype=np.float32)
    return np.clip(np.trunc(np.float32(255.0) * x), 0, 255).astype(np.float64)


def octave_sizes(H, W):
    """-> [(h, w)] of the octaves that are built: round(log2(min(2H, 2W)) - 2) + 1 of them, cut where one gets too small to detect in."""
    h, w = 2 * H, 2 * W
    n = int(_round(math.log2(min(h, w)) - 2)) + 1
    out = []
    for _ in range(max(n, 0)):
        if min(h, w) < MIN_SIDE:
            break
        out.append((h, w))
        h, w = h // 2, w // 2
    return out


def level_sigmas():
    """incremental blur of the 6 images of an octave; [0] is the blur of the upsampled base image"""
    sig = [math.sqrt(SIGMA * SIGMA - 1.0)]
    for i in range(1, S + 3):
        a, b = SIGMA * 2.0 ** ((i - 1) / S), SIGMA * 2.0 ** (i / S)
        sig.append(math.sqrt(b * b - a * a))
    return sig


def taps(sigma):
    """Gaussian taps: radius (round(8 sigma + 1) | 1) // 2, normalised in fp64, stored as fp32 (returned as float64)"""
    r = (int(_round(8.0 * sigma + 1.0)) | 1) // 2
    t = np.exp(-np.arange(-r, r + 1, dtype=np.float64) ** 2 / (2.0 * sigma * sigma))
    return (t / t.sum()).astype(np.float32).astype(np.float64)


def _reflect101(i, n):
    p = 2 * (n - 1)
    i = np.mod(i, p)
    return np.where(i >= n, p - i, i)


def blur(img, sigma):
    """separable Gaussian, rows then columns, reflect-101 borders (any number of bounces)"""
    t = taps(sigma)
    r = len(t) // 2
    h, w = img.shape
    cols = _reflect101(np.arange(-r, w + r), w)
    rows = _reflect101(np.arange(-r, h + r), h)
    p = img[:, cols]
    mid = sum(t[k] * p[:, k:k + w] for k in range(2 * r + 1))
    p = mid[rows, :]
    return sum(t[k] * p[k:k + h, :] for k in range(2 * r + 1))


def upsample2(u):
    """bilinear 2x, pixel-centre aligned: output j samples (j + 0.5) / 2 - 0.5, borders replicated"""
    def axis(a, ax):
        a = np.moveaxis(a, ax, 0)
        n = a.shape[0]
        lo = a[np.maximum(np.arange(n) - 1, 0)]
        hi = a[np.minimum(np.arange(n) + 1, n - 1)]
        out = np.empty((2 * n,) + a.shape[1:], dtype=np.float64)
        out[0::2] = 0.25 * lo + 0.75 * a
        out[1::2] = 0.75 * a + 0.25 * hi
        return np.moveaxis(out, 0, ax)
    return axis(axis(u, 0), 1)


def pyramid(u):
    """u [H, W] 8-bit values -> (gauss, dog): per octave arrays [6, h, w] and [5, h, w], float64"""
    H, W = u.shape
    sig = level_sigmas()
    gauss, dog = [], []
    for o, (h, w) in enumerate(octave_sizes(H, W)):
        g = np.empty((S + 3, h, w))
        g[0] = blur(upsample2(u), sig[0]) if o == 0 else gauss[-1][S][0:2 * h:2, 0:2 * w:2]
        for i in range(1, S + 3):
            g[i] = blur(g[i - 1], sig[i])
        gauss.append(g)
        dog.append(g[1:] - g[:-1])
    return gauss, dog


# ---------------------------------------------------------------- detect
def extrema(dog):
    """-> int [n, 4] (octave, layer, row, column): > 0 and >= all 26 neighbours, or < 0 and <= all of them; layers 1..S, 5-pixel border"""
    out = []
    for o, d in enumerate(dog):
        _, h, w = d.shape
        c = d[1:S + 1, BORDER:h - BORDER, BORDER:w - BORDER]
        mx = np.full(c.shape, -np.inf)
        mn = np.full(c.shape, np.inf)
        for dl in (-1, 0, 1):
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    if dl == dy == dx == 0:
                        continue
                    nb = d[1 + dl:S + 1 + dl, BORDER + dy:h - BORDER + dy, BORDER + dx:w - BORDER + dx]
                    mx = np.maximum(mx, nb)
                    mn = np.minimum(mn, nb)
        m = ((c > 0) & (c >= mx)) | ((c < 0) & (c <= mn))
        l, r, cc = np.nonzero(m)
        out.append(np.stack([np.full_like(l, o), l + 1, r + BORDER, cc + BORDER], axis=1))
    return np.concatenate(out) if out else np.zeros((0, 4), dtype=np.int64)


def refine(dog, cand):
    """cand int [n, 4] -> (ki int [m, 4] converged sample, kf float64 [m, 4] = x, y, size, response, src [m] index into cand).
    Up to 5 Newton steps on the 3-D quadratic in float64; the 3x3 system is solved by cofactors in a fixed operation order."""
    ki_out, kf_out, src = [], [], []
    for o, d in enumerate(dog):
        sel = np.nonzero(cand[:, 0] == o)[0]
        if sel.size == 0:
            continue
        d = np.asarray(d, dtype=np.float64)
        _, h, w = d.shape
        l, r, c = (cand[sel, k].astype(np.int64) for k in (1, 2, 3))
        alive = np.ones(sel.size, dtype=bool)
        done = np.zeros(sel.size, dtype=bool)
        res = np.zeros((sel.size, 4))
        for _ in range(MAX_STEPS):
            a = np.nonzero(alive & ~done)[0]
            if a.size == 0:
                break
            L, R, C = l[a], r[a], c[a]
            v = d[L, R, C]
            gx = 0.5 * (d[L, R, C + 1] - d[L, R, C - 1])
            gy = 0.5 * (d[L, R + 1, C] - d[L, R - 1, C])
            gs = 0.5 * (d[L + 1, R, C] - d[L - 1, R, C])
            v2 = 2.0 * v
            dxx = d[L, R, C + 1] + d[L, R, C - 1] - v2
            dyy = d[L, R + 1, C] + d[L, R - 1, C] - v2
            dss = d[L + 1, R, C] + d[L - 1, R, C] - v2
            dxy = 0.25 * (d[L, R + 1, C + 1] - d[L, R + 1, C - 1] - d[L, R - 1, C + 1] + d[L, R - 1, C - 1])
            dxs = 0.25 * (d[L + 1, R, C + 1] - d[L + 1, R, C - 1] - d[L - 1, R, C + 1] + d[L - 1, R, C - 1])
            dys = 0.25 * (d[L + 1, R + 1, C] - d[L + 1, R - 1, C] - d[L - 1, R + 1, C] + d[L - 1, R - 1, C])
            c00 = dyy * dss - dys * dys
            c01 = dxs * dys - dxy * dss
            c02 = dxy * dys - dxs * dyy
            c11 = dxx * dss - dxs * dxs
            c12 = dxy * dxs - dxx * dys
            c22 = dxx * dyy - dxy * dxy
            det = dxx * c00 + dxy * c01 + dxs * c02
            ok = det != 0.0
            with np.errstate(divide="ignore", invalid="ignore"):
                xc = -(c00 * gx + c01 * gy + c02 * gs) / det
                xr = -(c01 * gx + c11 * gy + c12 * gs) / det
                xl = -(c02 * gx + c12 * gy + c22 * gs) / det
            conv = ok & (np.abs(xc) < 0.5) & (np.abs(xr) < 0.5) & (np.abs(xl) < 0.5)
            big = ~(np.abs(xc) < 1e6) | ~(np.abs(xr) < 1e6) | ~(np.abs(xl) < 1e6)
            ok &= conv | ~big
            # converged: outputs
            k = a[conv]
            scale = 2.0 ** (o - 1)
            res[k, 0] = (C[conv] + xc[conv]) * scale - 0.25
            res[k, 1] = (R[conv] + xr[conv]) * scale - 0.25
            res[k, 2] = 2.0 * (SIGMA * np.exp2((L[conv] + xl[conv]) / 3.0) * scale)
            res[k, 3] = np.abs(v[conv] + 0.5 * (gx[conv] * xc[conv] + gy[conv] * xr[conv] + gs[conv] * xl[conv])) / 255.0
            done[k] = True
            # move on
            mv = ok & ~conv
            k = a[mv]
            c[k] += _round(xc[mv]).astype(np.int64)
            r[k] += _round(xr[mv]).astype(np.int64)
            l[k] += _round(xl[mv]).astype(np.int64)
            inside = (l[k] >= 1) & (l[k] <= S) & (c[k] >= BORDER) & (c[k] < w - BORDER) & (r[k] >= BORDER) & (r[k] < h - BORDER)
            alive[k[~inside]] = False
            alive[a[~ok]] = False
        k = np.nonzero(done)[0]
        ki_out.append(np.stack([np.full(k.size, o), l[k], r[k], c[k]], axis=1))
        kf_out.append(res[k])
        src.append(sel[k])
    if not ki_out:
        return np.zeros((0, 4), dtype=np.int64), np.zeros((0, 4)), np.zeros(0, dtype=np.int64)
    return np.concatenate(ki_out), np.concatenate(kf_out), np.concatenate(src)


EXITS = ("converged", "det0", "big", "border", "layer", "steps")


def refine_traced(dog, cand, max_steps=MAX_STEPS):
    """refine() one candidate at a time, saying how each ended -> per candidate (exit, steps, (l, r, c)): exit is one of EXITS,
    steps the number of Newton systems solved, (l, r, c) the sample it ended on (for "border" / "layer" the one it moved to and
    never read).  max_steps other than MAX_STEPS asks what a different step limit would have done.  "converged" with steps == 1
    is converged at once, with more it moved first; a move that leaves both the layers and the border is "layer".  The same operations in the same order as refine(), which it does not replace."""
    out = []
    for o, l, r, c in np.asarray(cand, dtype=np.int64).reshape(-1, 4).tolist():
        d = np.asarray(dog[o], dtype=np.float64)
        _, h, w = d.shape
        end = None
        for it in range(1, max_steps + 1):
            v = d[l, r, c]
            gx = 0.5 * (d[l, r, c + 1] - d[l, r, c - 1])
            gy = 0.5 * (d[l, r + 1, c] - d[l, r - 1, c])
            gs = 0.5 * (d[l + 1, r, c] - d[l - 1, r, c])
            v2 = 2.0 * v
            dxx = d[l, r, c + 1] + d[l, r, c - 1] - v2
            dyy = d[l, r + 1, c] + d[l, r - 1, c] - v2
            dss = d[l + 1, r, c] + d[l - 1, r, c] - v2
            dxy = 0.25 * (d[l, r + 1, c + 1] - d[l, r + 1, c - 1] - d[l, r - 1, c + 1] + d[l, r - 1, c - 1])
            dxs = 0.25 * (d[l + 1, r, c + 1] - d[l + 1, r, c - 1] - d[l - 1, r, c + 1] + d[l - 1, r, c - 1])
            dys = 0.25 * (d[l + 1, r + 1, c] - d[l + 1, r - 1, c] - d[l - 1, r + 1, c] + d[l - 1, r - 1, c])
            c00 = dyy * dss - dys * dys
            c01 = dxs * dys - dxy * dss
            c02 = dxy * dys - dxs * dyy
            c11 = dxx * dss - dxs * dxs
            c12 = dxy * dxs - dxx * dys
            c22 = dxx * dyy - dxy * dxy
            det = dxx * c00 + dxy * c01 + dxs * c02
            if det == 0.0:
                end = "det0"
                break
            with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
                xc = -(c00 * gx + c01 * gy + c02 * gs) / det
                xr = -(c01 * gx + c11 * gy + c12 * gs) / det
                xl = -(c02 * gx + c12 * gy + c22 * gs) / det
            if abs(xc) < 0.5 and abs(xr) < 0.5 and abs(xl) < 0.5:
                end = "converged"
                break
            if not abs(xc) < 1e6 or not abs(xr) < 1e6 or not abs(xl) < 1e6:
                end = "big"
                break
            c += int(_round(xc))
            r += int(_round(xr))
            l += int(_round(xl))
            if l < 1 or l > S:
                end = "layer"
                break
            if c < BORDER or c >= w - BORDER or r < BORDER or r >= h - BORDER:
                end = "border"
                break
        out.append((end or "steps", it, (l, r, c)))
    return out


def detect(dog):
    """DoG volume -> (ki, kf) in the order of the candidates: (octave, layer, row, column) of the extremum each started from"""
    ki, kf, _ = refine(dog, extrema(dog))
    return ki, kf


# ---------------------------------------------------------------- orient
def _sigma_oct(o, size):
    return np.float64(size) * 0.5 / 2.0 ** (o - 1)


def _gradients(img, y, x):
    dx = img[y, x + 1] - img[y, x - 1]
    dy = img[y + 1, x] - img[y - 1, x]
    return dx, dy


def orientation_histogram(gauss, k, size):
    """smoothed 36-bin histogram of keypoint k = (o, l, r, c) with cv2 size `size`"""
    o, l, r, c = (int(v) for v in k)
    img = gauss[o][l]
    h, w = img.shape
    sg = _sigma_oct(o, size)
    rad = int(_round(4.5 * sg))
    es = -1.0 / (2.0 * (1.5 * sg) ** 2)
    i, j = np.meshgrid(np.arange(-rad, rad + 1), np.arange(-rad, rad + 1), indexing="ij")
    y, x = r + i, c + j
    m = (y > 0) & (y < h - 1) & (x > 0) & (x < w - 1)
    i, j, y, x = i[m], j[m], y[m], x[m]
    dx, dy = _gradients(img, y, x)
    wgt = np.exp((i * i + j * j) * es)
    mag = np.sqrt(dx * dx + dy * dy)
    b = _round(np.degrees(np.arctan2(dy, dx)) * (ORI_BINS / 360.0)).astype(np.int64) % ORI_BINS
    raw = np.bincount(b, weights=wgt * mag, minlength=ORI_BINS)
    return (np.roll(raw, 2) + np.roll(raw, -2)) * (1.0 / 16) + (np.roll(raw, 1) + np.roll(raw, -1)) * (4.0 / 16) + raw * (6.0 / 16)


def orientation_bin_margin(gauss, k, size):
    """smallest distance, in bins, of the angle of any non-zero gradient in keypoint k's window from a histogram bin edge (0.5 when
    there is none): above the last-bit difference of two atan2, both sides put every sample into the same bin"""
    o, l, r, c = (int(v) for v in k)
    img = gauss[o][l]
    h, w = img.shape
    rad = int(_round(4.5 * _sigma_oct(o, size)))
    i, j = np.meshgrid(np.arange(-rad, rad + 1), np.arange(-rad, rad + 1), indexing="ij")
    y, x = r + i, c + j
    m = (y > 0) & (y < h - 1) & (x > 0) & (x < w - 1)
    dx, dy = _gradients(img, y[m], x[m])
    nz = (dx != 0) | (dy != 0)
    if not nz.any():
        return 0.5
    t = np.degrees(np.arctan2(dy[nz], dx[nz])) * (ORI_BINS / 360.0) + 0.5
    return float(np.min(np.abs(t - np.round(t))))


def histogram_peaks(hist):
    """-> [(angle in degrees, height, near)] by descending height: local peaks >= 0.8 max, parabolic interpolation; `near` is the
    relative distance of the weakest decision about this histogram from the 0.8 line (for the tests' exemption rule)"""
    mx = hist.max()
    left, right = np.roll(hist, 1), np.roll(hist, -1)
    local = (hist > left) & (hist > right)
    near = np.min(np.abs(hist[local] - 0.8 * mx) / mx) if mx > 0 and local.any() else np.inf
    out = []
    for j in np.nonzero(local & (hist >= 0.8 * mx))[0]:
        b = j + 0.5 * (left[j] - right[j]) / (left[j] - 2.0 * hist[j] + right[j])
        b = b + ORI_BINS if b < 0 else (b - ORI_BINS if b >= ORI_BINS else b)
        out.append((b * (360.0 / ORI_BINS), hist[j], j))
    out.sort(key=lambda t: (-t[1], t[2]))
    return [(a, hgt) for a, hgt, _ in out], near


def orient(gauss, ki, kf, upright=False):
    """-> (oi int [m, 6] = octave, layer, row, column, orientation rank, source keypoint; of float32 [m, 5] = x, y, size, angle,
    response; near [n] per source keypoint).  One keypoint per histogram peak, by descending peak height."""
    oi, of, near = [], [], np.full(len(ki), np.inf)
    kf32 = np.asarray(kf, dtype=np.float64).astype(np.float32)
    for n in range(len(ki)):
        if upright:
            peaks = [(0.0, 0.0)]
        else:
            peaks, near[n] = histogram_peaks(orientation_histogram(gauss, ki[n], kf32[n, 2]))
        for rank, (ang, _) in enumerate(peaks):
            ang = np.float32(ang)
            oi.append(list(ki[n]) + [rank, n])
            of.append([kf32[n, 0], kf32[n, 1], kf32[n, 2], np.float32(0.0) if ang >= np.float32(360.0) else ang, kf32[n, 3]])
    return (np.asarray(oi, dtype=np.int64).reshape(-1, 6), np.asarray(of, dtype=np.float32).reshape(-1, 5), near)


# ---------------------------------------------------------------- describe
def raw_descriptor(gauss, k, size, angle):
    """the 4 x 4 x 8 histogram (element order [row bin][column bin][orientation bin]) before normalisation"""
    o, l, r, c = (int(v) for v in k[:4])
    img = gauss[o][l]
    h, w = img.shape
    hw = 3.0 * _sigma_oct(o, size)
    rad = int(_round(hw * math.sqrt(2.0) * (D + 1) * 0.5))
    rad = min(rad, int(math.sqrt(float(h) * h + float(w) * w)))
    th = math.radians(float(angle))
    ct, st = math.cos(th) / hw, math.sin(th) / hw
    i, j = np.meshgrid(np.arange(-rad, rad + 1), np.arange(-rad, rad + 1), indexing="ij")
    crot = j * ct + i * st
    rrot = -j * st + i * ct
    rbin, cbin = rrot + D / 2 - 0.5, crot + D / 2 - 0.5
    y, x = r + i, c + j
    m = (rbin > -1) & (rbin < D) & (cbin > -1) & (cbin < D) & (y > 0) & (y < h - 1) & (x > 0) & (x < w - 1)
    rbin, cbin, crot, rrot, y, x = rbin[m], cbin[m], crot[m], rrot[m], y[m], x[m]
    dx, dy = _gradients(img, y, x)
    obin = (np.degrees(np.arctan2(dy, dx)) - float(angle)) * (NB / 360.0)
    mag = np.sqrt(dx * dx + dy * dy) * np.exp((crot * crot + rrot * rrot) * (-1.0 / (D * D * 0.5)))
    r0, c0, o0 = np.floor(rbin), np.floor(cbin), np.floor(obin)
    fr, fc, fo = rbin - r0, cbin - c0, obin - o0
    r0, c0, o0 = r0.astype(np.int64), c0.astype(np.int64), o0.astype(np.int64)
    hist = np.zeros(D * D * NB)
    for dr in (0, 1):
        for dc in (0, 1):
            for do in (0, 1):
                rr, cc, oo = r0 + dr, c0 + dc, (o0 + do) % NB
                ok = (rr >= 0) & (rr < D) & (cc >= 0) & (cc < D)
                v = mag * (fr if dr else 1 - fr) * (fc if dc else 1 - fc) * (fo if do else 1 - fo)
                hist += np.bincount(((rr * D + cc) * NB + oo)[ok], weights=v[ok], minlength=D * D * NB)
    return hist


def finish_descriptor(hist, quantize=True):
    """L2-normalise, clip at 0.2, renormalise; with quantize min(255, round(512 v)).  An all-zero histogram stays zero."""
    n = math.sqrt(float(np.sum(hist * hist)))
    if n == 0.0:
        return np.zeros_like(hist)
    v = np.minimum(hist / n, 0.2)
    v = v / math.sqrt(float(np.sum(v * v)))
    return np.minimum(255.0, _round(512.0 * v)) if quantize else v


def normalize_descriptors(desc, rootsift=True):
    """the reference's normalize_descriptors (base.py:27), except that an all-zero row stays zero"""
    desc = np.asarray(desc, dtype=np.float64)
    n = np.abs(desc).sum(axis=1, keepdims=True) if rootsift else np.sqrt((desc * desc).sum(axis=1, keepdims=True))
    out = desc / np.where(n == 0, 1.0, n)
    return np.sqrt(out) if rootsift else out


def describe(gauss, oi, of, quantize=True, rootsift=True):
    """-> float64 [m, 128] final descriptors of the oriented keypoints"""
    out = np.zeros((len(oi), D * D * NB))
    for n in range(len(oi)):
        out[n] = finish_descriptor(raw_descriptor(gauss, oi[n], of[n, 2], of[n, 3]), quantize)
    return normalize_descriptors(out, rootsift)


# ---------------------------------------------------------------- select
def sort_keys(oi):
    """(octave, layer, row, column, orientation rank) as one integer: the order of equal responses"""
    oi = np.asarray(oi, dtype=np.int64)
    return (((oi[:, 0] * 4 + oi[:, 1]) * 65536 + oi[:, 2]) * 65536 + oi[:, 3]) * 32 + oi[:, 4]


def select(xy, response, keys, nms_diameter, max_keypoints):
    """the reference's detect_kpts_opencv (greedy radius NMS in descending response with the distance <= r test, then the top
    max_keypoints) -> indices of the kept keypoints in output order: descending float32 response, equal ones by key, then index"""
    xy = np.asarray(xy, dtype=np.float32).astype(np.float64)
    resp = np.asarray(response, dtype=np.float32)
    n = len(resp)
    order = np.lexsort((np.arange(n), np.asarray(keys), -resp.astype(np.float64)))
    radius = nms_diameter / 2.0
    if radius > 0 and n:
        cell = max(radius, 1e-9)
        g = np.floor(xy / cell).astype(np.int64)
        buckets = {}
        for i in range(n):
            buckets.setdefault((g[i, 0], g[i, 1]), []).append(i)
        removed = np.zeros(n, dtype=bool)
        kept = []
        r2 = radius * radius
        for i in order:
            if removed[i]:
                continue
            kept.append(i)
            for gx in (g[i, 0] - 1, g[i, 0], g[i, 0] + 1):
                for gy in (g[i, 1] - 1, g[i, 1], g[i, 1] + 1):
                    for j in buckets.get((gx, gy), ()):
                        d = xy[j] - xy[i]
                        if d[0] * d[0] + d[1] * d[1] <= r2:
                            removed[j] = True
        order = np.asarray(kept, dtype=np.int64)
    if max_keypoints > 0:
        order = order[:max_keypoints]
    return order


def lafs_from_keypoints(of, mr_size=6.0):
    """the reference's lafs_from_opencv_kpts (base.py:52): scale mr_size * size, angle deg2rad(-angle).  In float32 operation by
    operation, as the reference computes it: at an angle of 6 rad one float32 rounding of the angle moves an entry of a LAF of scale
    100 by 5e-5, so a float64 evaluation would not be the reference's LAF to better than that."""
    of = np.asarray(of, dtype=np.float32)
    s = np.float32(mr_size) * of[:, 2]
    a = np.deg2rad(-of[:, 3])
    lafs = np.empty((len(of), 2, 3), dtype=np.float32)
    lafs[:, 0, 0], lafs[:, 0, 1], lafs[:, 0, 2] = s * np.cos(a), s * np.sin(a), of[:, 0]
    lafs[:, 1, 0], lafs[:, 1, 1], lafs[:, 1, 2] = -(s * np.sin(a)), s * np.cos(a), of[:, 1]
    return lafs.astype(np.float64)


def extract(image, max_keypoints=-1, nms_diameter=9.0, rootsift=True, upright=False, quantize_desc=True):
    """one image [H, W] in [0, 1] -> (lafs [n, 2, 3], scores [n], descriptors [n, 128], oi, of): the whole extractor.  Selection
    runs before the descriptors (it does not depend on them), so only the kept keypoints are described."""
    gauss, dog = pyramid(quantize(image))
    ki, kf = detect(dog)
    oi, of, _ = orient(gauss, ki, kf, upright)
    keep = select(of[:, :2], of[:, 4], sort_keys(oi), nms_diameter, max_keypoints)
    oi, of = oi[keep], of[keep]
    return lafs_from_keypoints(of), of[:, 4].astype(np.float64), describe(gauss, oi, of, quantize_desc, rootsift), oi, of


# ---------------------------------------------------------------- inputs of the selection fixture
def synthetic_keypoints(n, seed, H=120, W=160):
    """seeded cv2.KeyPoint fields for tests/golden/sift_select.npz: float32 [n, 5] = x, y, size, angle, response (responses distinct)
    and byte-valued descriptors float32 [n, 128]; regenerated by the tests instead of being stored"""
    i = np.arange(n, dtype=np.int64)
    h = lambda a, m: ((i * a + (i * i) % 7919 * 31 + seed * 977 + 12345) % m).astype(np.float64)      # integer hashes: no RNG stream to depend on
    of = np.empty((n, 5), dtype=np.float32)
    of[:, 0] = h(7919, 100003) / 100003 * (W - 1)
    of[:, 1] = h(104729, 99991) / 99991 * (H - 1)
    of[:, 2] = 2.0 + h(31, 1009) / 1009 * 30.0
    of[:, 3] = h(17, 3600) / 10.0
    order = (i * 7901 + seed) % max(n, 1) if math.gcd(7901, max(n, 1)) == 1 else i
    of[:, 4] = ((order + 1) / (n + 1.0)).astype(np.float32) * 0.2
    assert len(np.unique(of[:, 4])) == n
    j = np.arange(128, dtype=np.int64)
    desc = ((i[:, None] * 131 + j[None, :] * 71 + (i[:, None] * j[None, :]) % 97 + seed) % 256).astype(np.float32)
    desc[:, 5] += 1.0          # no all-zero row: the reference divides by the norm
    return of, desc
