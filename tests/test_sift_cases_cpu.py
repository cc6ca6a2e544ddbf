"""tests/sift_cases.py on the CPU: under the float64 restatement (tests/sift_ref.py) every crafted input reaches the edge it names.
Detect cases are traced with sift_ref.refine_traced (which exit each candidate takes, after how many steps), orient cases are held
to their peak counts, ties, wrap side and margins, overflow cases to their counts against the capacities.  No GPU.  Run with -s to
see what every case reaches."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sift_cases as C  # noqa: E402
import sift_ref as R  # noqa: E402

DETECT = {c.name: c for c in C.detect_cases()}
ORIENT = {c.name: c for c in C.orient_cases()}
DESCRIBE = {c.name: c for c in C.describe_cases()}
SELECT = {c.name: c for c in C.select_cases()}
BIN_MARGIN = 1e-6            # bins: far above the last-bit difference of two atan2
NEAR = 1e-3                  # relative distance of every peak decision from the 0.8 line


def _f64(vols):
    return [v.astype(np.float64) for v in vols]


def _traced(dog):
    d = _f64(dog)
    cand = R.extrema(d)
    return cand, R.refine_traced(d, cand)


# ---------------------------------------------------------------- the restatement's own tracer
@pytest.mark.parametrize("name", [n for n in DETECT if not n.startswith("checkerboard-24")])
def test_traced_refine_is_refine(name):
    """the candidates that refine_traced calls converged are the ones refine returns, on the samples it returns"""
    c = DETECT[name]
    for dog in c.dog:
        d = _f64(dog)
        cand = R.extrema(d)
        ki, _, src = R.refine(d, cand)
        tr = R.refine_traced(d, cand)
        conv = [i for i, t in enumerate(tr) if t[0] == "converged"]
        assert conv == src.tolist()
        assert [tr[i][2] for i in conv] == [tuple(k[1:]) for k in ki.tolist()]
        assert all(t[0] in R.EXITS and 1 <= t[1] <= R.MAX_STEPS for t in tr)


# ---------------------------------------------------------------- detect
@pytest.mark.parametrize("name", list(DETECT))
def test_detect_case_reaches_its_edge(name):
    c = DETECT[name]
    assert len(C.zero_dog(c.H, c.W)) == len(c.dog[0])
    for b, dog in enumerate(c.dog):
        for d, (h, w) in zip(dog, R.octave_sizes(c.H, c.W)):
            assert d.dtype == np.float32 and d.shape == (5, h, w)
            assert np.array_equal(d, np.round(d)) and np.abs(d).max() < 2.0 ** 23          # integers that fp32 holds exactly
        cand, tr = _traced(dog)
        look = {tuple(k): t for k, t in zip(cand.tolist(), tr)}
        kept = sum(t[0] == "converged" for t in tr)
        print(f"{name} image {b}: {len(cand)} candidates, {kept} kept, exits "
              f"{ {e: sum(t[0] == e for t in tr) for e in R.EXITS if any(t[0] == e for t in tr)} } -- {c.edge}")
        if c.candidates is not None:
            assert len(cand) == c.candidates[b]
        if c.kept is not None:
            assert kept == c.kept[b]
        for bb, k, ex, steps in c.claims:
            if bb == b:
                assert k in look, (name, k)
                assert look[k][0] == ex and (steps is None or look[k][1] == steps), (name, k, look[k])


def test_detect_cases_cover_every_exit_and_edge():
    seen, moved = set(), set()
    cols, rows, layers, octaves = set(), set(), set(), set()
    for c in DETECT.values():
        if c.name.startswith("checkerboard"):
            continue
        for dog in c.dog:
            d = _f64(dog)
            cand, tr = _traced(dog)
            for k, (ex, steps, end) in zip(cand.tolist(), tr):
                seen.add(ex)
                if ex == "converged" and steps > 1:
                    moved.add("layer" if end[0] != k[1] else "plane")
                if ex == "converged":
                    h, w = d[k[0]].shape[1:]
                    octaves.add((c.name, k[0]))
                    layers.add(end[0])
                    rows |= {"first"} if end[1] == R.BORDER else ({"last"} if end[1] == h - R.BORDER - 1 else set())
                    cols |= {"first"} if end[2] == R.BORDER else ({"last"} if end[2] == w - R.BORDER - 1 else set())
                    if w > C.SEG:
                        cols.add(end[2])
    assert seen == set(R.EXITS)
    assert moved == {"plane", "layer"}
    assert {"first", "last", C.SEG - 1, C.SEG, C.SEG + 1} <= cols and rows == {"first", "last"} and layers == {1, 2, 3}
    assert {(("geometry-octaves"), o) for o in range(3)} <= octaves


def test_detect_special_cases():
    # the tie pair sees offsets of exactly +-0.5; with `<= 0.5` both would converge
    c = DETECT["tie-pair"]
    cand, tr = _traced(c.dog[0])
    assert [t[:2] for t in tr] == [("steps", 5)] * 2 and tr[0][2] == tr[1][2] == (2, 8, 8)
    # the zero extrema: below (above) all 26 neighbours, which are all positive (negative); not candidates, and would converge at once
    d = _f64(DETECT["zero-extrema"].dog[0])[0]
    for (r, col), sign in (((7, 7), 1.0), ((10, 10), -1.0)):
        nb = np.delete(d[1:4, r - 1:r + 2, col - 1:col + 2].reshape(-1), 13) * sign
        assert d[2, r, col] == 0.0 and (nb > 0).all()
        assert [0, 2, r, col] not in R.extrema([d]).tolist()
        assert R.refine_traced([d], np.array([[0, 2, r, col]]))[0] == ("converged", 1, (2, r, col))
    # five steps used up, where six would converge; a fifth step that converges
    c = DETECT["sixth-step"]
    k = np.array([[0, 1, 14, 14]])
    assert R.refine_traced(_f64(c.dog[0]), k)[0][:2] == ("steps", 5)
    assert R.refine_traced(_f64(c.dog[0]), k, max_steps=6)[0][:2] == ("converged", 6)
    assert any(t[:2] == ("converged", 5) for t in _traced(DETECT["fifth-step"].dog[0])[1])
    # the long moves land where they say: the first column outside the border on either side, a layer above 3 and one below 1
    cand, tr = _traced(DETECT["long-moves"].dog[0])
    ends = {tuple(k[1:]): t[2] for k, t in zip(cand.tolist(), tr)}
    assert ends[(2, 12, 24)][2] == 32 - R.BORDER and ends[(2, 22, 7)][2] == R.BORDER - 1
    assert ends[(2, 16, 16)][0] > R.S and ends[(2, 22, 22)][0] < 1
    assert ends[(2, 8, 26)][2] >= 32 - R.BORDER and ends[(2, 16, 5)][2] < R.BORDER
    assert ends[(2, 26, 12)][1] >= 32 - R.BORDER and ends[(2, 5, 20)][1] < R.BORDER
    # moved onto the border: the landing sample is the one that converges when the block lies 12 columns further left
    assert _traced(DETECT["moved-onto-border"].dog[0])[1][4][2] == (1, 18, 32 - R.BORDER)
    # the move onto layer 3 converges there
    look = {tuple(k): t for k, t in zip(*[x if i else x.tolist() for i, x in enumerate(_traced(DETECT["moved-to-layer3"].dog[0]))])}
    assert look[(0, 2, 15, 19)] == ("converged", 2, (3, 15, 19))
    # the big stencil's offsets are over the 1e6 line, far from it
    s = C.big_stencil()
    gx, dxx, dxy = 0.5 * (s[1, 1, 2] - s[1, 1, 0]), s[1, 1, 2] + s[1, 1, 0] - 2 * s[1, 1, 1], 0.25 * (s[1, 2, 2] - s[1, 2, 0] - s[1, 0, 2] + s[1, 0, 0])
    dyy = s[1, 2, 1] + s[1, 0, 1] - 2 * s[1, 1, 1]
    assert abs(dyy * gx / (dxx * dyy - dxy * dxy)) > 2e6


def test_checkerboard_overflows_and_fills():
    for H, W, n in ((16, 16, 1040), (24, 24, 3288), (24, 40, 6200)):
        assert C.checkerboard_count(H, W) == n
    cap, cap2, capn = C.capacities(16, 16)
    assert (cap, cap2, capn) == (1024, 1280, 40960) == C.capacities(8, 8) == C.capacities(24, 40)
    c = DETECT["checkerboard-16x16"]
    ki, kf = R.detect(_f64(c.dog[0]))
    assert len(ki) == 1040 > cap and np.all(kf[:, 3] == 16.0 / 255.0)
    assert np.array_equal(ki, R.extrema(_f64(c.dog[0])))                              # every candidate converges at once
    # more than one workgroup row of candidates: octave 0 holds 968 of them, 22 in every (layer, row); cap is passed inside octave 1
    assert (ki[:, 0] == 0).sum() == 968 and len(R.detect(_f64(c.dog[1]))[0]) == 4
    ki, _ = R.detect(_f64(DETECT["checkerboard-24x40"].dog[0]))
    assert len(ki) == 6200 and len(np.unique(ki[:, 0])) == 3
    full = R.detect(_f64(C.checkerboard_full()))[0]
    assert len(full) == cap                                                           # exactly full, no overflow


# ---------------------------------------------------------------- orient
def _hist(c, n):
    g = _f64(c.gauss)
    size = np.float32(c.kf[n, 2])
    return R.orientation_histogram(g, c.ki[n], size), R.orientation_bin_margin(g, c.ki[n], size)


def _raw_peak_bins(hist):
    """(bin, interpolated bin before the wrap) of every local peak over the 0.8 line"""
    left, right = np.roll(hist, 1), np.roll(hist, -1)
    ok = (hist > left) & (hist > right) & (hist >= 0.8 * hist.max())
    return [(int(j), j + 0.5 * (left[j] - right[j]) / (left[j] - 2.0 * hist[j] + right[j])) for j in np.nonzero(ok)[0]]


@pytest.mark.parametrize("name", list(ORIENT))
def test_orient_case_reaches_its_edge(name):
    c = ORIENT[name]
    for n in range(len(c.ki)):
        o, l, r, col = c.ki[n]
        h, w = c.gauss[o].shape[1:]
        assert 1 <= l <= R.S and R.BORDER <= r < h - R.BORDER and R.BORDER <= col < w - R.BORDER
        hist, margin = _hist(c, n)
        peaks, near = R.histogram_peaks(hist)
        hs = sorted(hgt for _, hgt in peaks)
        gaps = [b - a for a, b in zip(hs, hs[1:])]
        print(f"{name} keypoint {n}: {len(peaks)} peaks at {[round(a, 4) for a, _ in peaks]}, near {near:.3g}, bin margin {margin:.3g} -- {c.edge}")
        assert margin >= BIN_MARGIN and near >= NEAR
        assert len(peaks) <= C.MAX_PEAKS
        # two peaks are exactly as high as each other or apart by far more than the 2^-40 the kernel's fixed point resolves
        assert all(g == 0.0 or g > 1e-9 * hist.max() for g in gaps), gaps
        if c.peaks is not None:
            assert len(peaks) == c.peaks[n]


def test_orient_special_cases():
    c = ORIENT["two-peaks"]
    peaks, _ = R.histogram_peaks(_hist(c, 0)[0])
    assert [round(a) for a, _ in peaks] == [180, 0] and 0.8 < peaks[1][1] / peaks[0][1] < 0.95          # by height, against bin order
    for name, angles in (("two-peaks-tie", [0.0, 180.0]), ("four-tie", [0.0, 90.0, 180.0, 270.0])):
        peaks, _ = R.histogram_peaks(_hist(ORIENT[name], 0)[0])
        assert [a for a, _ in peaks] == angles and len({hgt for _, hgt in peaks}) == 1                 # exact ties, in bin order
    # the wrap: bin 0 interpolates below 0; in wrap-to-zero so little that float32 rounds the angle to 360, which becomes 0
    for name, lo, hi in (("wrap-negative", -0.5, -1e-3), ("wrap-to-zero", -1e-6, -1e-12), ("wrap-positive", 1e-3, 0.5)):
        c = ORIENT[name]
        raw = dict(_raw_peak_bins(_hist(c, 0)[0]))
        assert lo < raw[0] < hi, (name, raw[0])
        _, of, _ = R.orient(_f64(c.gauss), c.ki, c.kf)
        a = float(of[np.argmin(np.abs((of[:, 3] + 180.0) % 360.0 - 180.0)), 3])
        if name == "wrap-negative":
            assert 355.0 < a < 360.0
        elif name == "wrap-to-zero":
            assert a == 0.0 and np.float32((raw[0] + 36.0) * 10.0) == np.float32(360.0)
        else:
            assert 0.0 < a < 5.0
    assert len(R.histogram_peaks(_hist(ORIENT["cone"], 0)[0])[0]) == 6
    peaks, _ = R.histogram_peaks(_hist(ORIENT["facets"], 0)[0])                        # the case that comes closest to SIFT_MAX_PEAKS
    assert len(peaks) == 11 > C.MAX_PEAKS // 2 and len({hgt for _, hgt in peaks}) == 11
    assert max(len(R.histogram_peaks(_hist(c, n)[0])[0]) for c in ORIENT.values() for n in range(len(c.ki))) == 11
    # windows cut by the image edge on all four sides
    c = ORIENT["cut-windows"]
    cut = set()
    for n in range(len(c.ki)):
        _, _, r, col = c.ki[n]
        rad = int(R._round(4.5 * float(np.float32(c.kf[n, 2]))))
        cut |= {s for s, hit in (("top", r - rad <= 0), ("bottom", r + rad >= 31), ("left", col - rad <= 0), ("right", col + rad >= 31)) if hit}
    assert cut == {"top", "bottom", "left", "right"}
    # no gradient: an all-zero histogram, no peak, no oriented keypoint -- and the neighbours of such a keypoint keep theirs
    c = ORIENT["no-gradient"]
    assert not _hist(c, 0)[0].any() and len(R.orient(_f64(c.gauss), c.ki, c.kf)[0]) == 0
    c = ORIENT["no-gradient-between"]
    assert R.orient(_f64(c.gauss), c.ki, c.kf)[0][:, 5].tolist() == [0] * 4 + [2] * 4
    # upright: one keypoint each at angle 0, whatever the histogram says
    oi, of, _ = R.orient(_f64(c.gauss), c.ki, c.kf, upright=True)
    assert oi[:, 5].tolist() == [0, 1, 2] and not of[:, 3].any()


def test_orient_overflow_input():
    H, W, gauss, ki, kf = C.two_peak_overflow()
    cap, cap2, _ = C.capacities(H, W)
    oi, of, near = R.orient(_f64(gauss[0]), ki[0][:1], kf[0][:1])
    assert len(ki[0]) == cap and len(oi) == 2 and 2 * cap == 2048 > cap2
    assert R.orientation_bin_margin(_f64(gauss[0]), ki[0][0], np.float32(kf[0][0, 2])) >= BIN_MARGIN and near[0] >= NEAR
    oi, _, near = R.orient(_f64(gauss[1]), ki[1], kf[1])
    assert oi[:, 5].tolist() == [0] * 4 and near[0] >= NEAR


# ---------------------------------------------------------------- describe
def test_describe_cases_reach_their_edges():
    c = DESCRIBE["constant"]
    assert c.zero and not R.describe(_f64(c.gauss), c.oi, c.of, False, True).any()
    assert not R.describe(_f64(c.gauss), c.oi, c.of, True, False).any()
    for name, n in (("axes-four-tie", 4), ("axes-two-peaks-tie", 2)):
        c = DESCRIBE[name]
        assert len(c.oi) == n and all(float(a) % 90.0 == 0.0 for a in c.of[:, 3])
        g = _f64(c.gauss)[0][int(c.oi[0, 1])]
        dx, dy = g[1:-1, 2:] - g[1:-1, :-2], g[2:, 1:-1] - g[:-2, 1:-1]
        assert not ((dx != 0) & (dy != 0)).any() and (dx != 0).any()                  # every gradient lies along an axis
    c = DESCRIBE["corners-smallest-octave"]
    o = int(c.oi[0, 0])
    h, w = c.gauss[o].shape[1:]
    assert o == len(c.gauss) - 1 and (h, w) == (12, 16)
    assert {(int(r), int(col)) for r, col in c.oi[:, 2:4]} == {(5, 5), (5, w - 6), (h - 6, 5), (h - 6, w - 6)}
    for n in range(len(c.oi)):
        rad, diag = C.describe_radius(c, n)
        assert rad > diag == 20                                                       # the clamp engages
        assert int(c.oi[n, 2]) - diag <= 0 and int(c.oi[n, 3]) + diag >= w - 1       # and the clamped window still crosses the border
    d = R.describe(_f64(c.gauss), c.oi, c.of, False, True)
    assert (np.abs(d).max(axis=1) > 0.05).all()


# ---------------------------------------------------------------- select
def _entries(of, diameter):
    """NMS neighbour entries: pairs of points within the radius (float32 positions, distance in float64)"""
    if diameter <= 0 or len(of) == 0:
        return 0
    xy = of[:, :2].astype(np.float64)
    d2 = ((xy[:, None, :] - xy[None, :, :]) ** 2).sum(-1)
    return int((np.triu(d2 <= (diameter / 2.0) ** 2, 1)).sum())


@pytest.mark.parametrize("name", list(SELECT))
def test_select_case_reaches_its_edge(name):
    c = SELECT[name]
    cap, cap2, capn = C.capacities(c.H, c.W)
    over = []
    for b, (of, keys) in enumerate(zip(c.of, c.keys)):
        assert len(of) <= cap2 and of.dtype == np.float32
        e = _entries(of, c.diameter)
        keep = R.select(of[:, :2], of[:, 4], R.sort_keys(keys), c.diameter, c.max_kpts)
        print(f"{name} image {b}: {len(of)} points, {e} entries of {capn}, {len(keep)} kept -- {c.edge}")
        over.append(e > capn)
        if c.entries is not None:
            assert e == c.entries[b]
        if c.kept is not None and not over[-1]:
            assert len(keep) == c.kept[b]
    assert any(over) == c.overflow
    if c.overflow:
        assert over[0] and not over[-1] and len(c.of) == 2 and c.kept[0] == 0        # image 0 overflows, never the last one


def test_select_special_cases():
    cap, cap2, capn = C.capacities(8, 8)
    assert C.pairs(286) == 40755 <= capn < C.pairs(300) == 44850 and C.pairs(190) + C.pairs(215) == capn
    assert len(SELECT["distinct-1280"].of[0]) == cap2
    for n in (1, 255, 256, 257, 1280):
        assert len(np.unique(SELECT[f"distinct-{n}"].of[0][:, 4])) == n
    # the cut falls inside a run of equal responses, so the key decides who is kept
    for k in (50, 150, 299):
        c = SELECT[f"equal-run-cut-{k}"]
        resp = np.sort(c.of[0][:, 4])[::-1]
        assert resp[k - 1] == resp[k]
    c = SELECT["empty-beside-many"]
    assert len(c.of[0]) == 0 and len(c.of[1]) == 300


# ---------------------------------------------------------------- inputs of the overflow chains on the GPU
def test_ramp_and_dense_image():
    """the plane of constant gradient that follows the overflowed detect puts every sample far from a bin edge and gives one peak;
    the dot lattice that the module-level tests feed has over 600 orientations, so that with a radius spanning the image its
    n (n - 1) / 2 neighbour entries pass the 32 * cap2 there is room for by more than a factor of two"""
    planes = [np.stack([C.ramp(h, w)] * 6) for h, w in R.octave_sizes(16, 16)]
    ki, kf = R.detect(_f64(C.checkerboard(16, 16)))
    oi, _, near = R.orient(planes, ki[::37], kf[::37])
    assert len(oi) == len(ki[::37]) and near.min() >= NEAR
    assert min(R.orientation_bin_margin(planes, k, np.float32(f[2])) for k, f in zip(ki[::37], kf[::37])) >= 0.1
    img = np.zeros((96, 96))
    img[5::10, 5::10] = 1.0
    gauss, dog = R.pyramid(R.quantize(img))
    ki, kf = R.detect(dog)
    oi, _, _ = R.orient(gauss, ki, kf)
    cap, cap2, capn = C.capacities(96, 96)
    print(f"dense image: {len(ki)} keypoints, {len(oi)} oriented, {C.pairs(len(oi))} pairs against {capn}")
    assert len(ki) <= cap and len(oi) <= cap2 and C.pairs(len(oi)) > 2 * capn
    assert len(oi) >= 3 * len(ki)                    # about four orientations per dot: the margin does not hang on one of them
