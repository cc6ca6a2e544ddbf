"""tests/superpoint_detect_cases.py on the CPU: every crafted heatmap reaches the edge it names under the float64 restatement
(superpoint_ref.select / pixel_decisions), the restatement agrees with a second implementation written as loops over pixels and, where
kornia is installed, with the reference's own chain of library calls on CPU torch; the describe inputs reach taps outside the coarse map
on every side and in every corner.  Run with -s to see, per case, the candidate counts and the edge reached."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import superpoint_detect_cases as cases
import superpoint_ref as R
from openglue_amd import _lib

NAMES = list(cases.CASES)


def _select(c):
    return R.select(c.heat.double(), c.k, c.border, cases.thr32(c.thr), c.max_kpts)


def _bits(t):
    return t.contiguous().view(torch.int32)


# ---------------------------------------------------------------- the edge is reached
@pytest.mark.parametrize("name", NAMES)
def test_edge_reached(name):
    c = cases.CASES[name]
    B, Hh, Wh = c.heat.shape
    r = (c.k - 1) // 2
    assert 8 <= Hh <= 32 and Wh <= 776
    keep, _ = R.pixel_decisions(c.heat.double(), c.k, c.border, cases.thr32(c.thr))
    sel = _select(c)
    n_cand = [s["n_cand"] for s in sel]
    m = len(sel[0]["idx"])
    print(f"{name}: n_cand {n_cand}, kept {m}, order {[s['order'] for s in sel]} -- {c.edge}")
    assert n_cand == [int(keep[b].sum()) for b in range(B)] and all(len(s["idx"]) == m for s in sel)
    for b, y, x in c.kept:
        assert bool(keep[b, y, x]), (name, "kept", b, y, x)
    for b, y, x in c.dropped:
        assert not bool(keep[b, y, x]), (name, "dropped", b, y, x)
    for group in c.ties:
        v = torch.stack([c.heat[p] for p in group])
        assert len(group) > 1 and bool((_bits(v) == _bits(v)[0]).all()), (name, group)
    if c.n_cand is not None:
        assert n_cand == c.n_cand, name
    if c.m is not None:
        assert m == c.m, name
    if c.order is not None:
        assert [s["order"] for s in sel] == c.order, name
    # the selection never outgrows the buffer that SuperPointNet.detect allocates from og_superpoint_capacity
    cap = _lib.load().og_superpoint_capacity(Hh, Wh, c.max_kpts)
    assert m <= cap and (c.max_kpts <= 0 or cap <= c.max_kpts) and max(n_cand) <= _lib.load().og_superpoint_capacity(Hh, Wh, -1), name

    family = name.split("-")[0]
    if family == "seam":
        seams = list(range(cases.SEG, Wh, cases.SEG))
        assert seams and all(any(x == x0 + d and b == 0 for b, _, x in c.kept) for x0 in seams for d in (-1, 0, 1))
        for x0 in seams:                                     # the pairs of image 1 straddle the seam, at distance r, r and r + 1
            rows = {y: sorted(x for b, yy, x in c.kept + c.dropped if b == 1 and yy == y and abs(x - x0) <= r + 1) for y in (3, 12, 21)}
            assert all(len(v) == 2 and v[0] < x0 <= v[1] for v in rows.values()), rows
            assert [v[1] - v[0] for v in rows.values()] == [r, r, r + 1]
            xl, xr = rows[3]
            assert c.heat[1, 3, xr] > c.heat[1, 3, xl] and c.heat[1, 12, xl] > c.heat[1, 12, xr]
            # filler candidates whose window crosses the seam, on both sides of it
            assert int(keep[:, :, x0 - r:x0].sum()) > 0 and int(keep[:, :, x0:x0 + r].sum()) > 0
    if family == "plateau":
        (a, b2), (p, q), (u, v), block = c.ties
        cheb = lambda s, t: max(abs(s[1] - t[1]), abs(s[2] - t[2]))
        assert cheb(a, b2) == 1 and cheb(p, q) == r and cheb(u, v) == r + 1 and len(block) == 9
    if family == "edge_replicate":
        assert c.border == 0 and float(c.heat.max()) == float(c.heat[0, 0, 0])
        rim = torch.zeros(Hh, Wh, dtype=torch.bool)
        rim[0], rim[-1], rim[:, 0], rim[:, -1] = True, True, True, True
        assert int((keep[0] & rim).sum()) == 0                       # no pixel of the rim is ever kept
        for _, y, x in c.dropped:                                    # each is the strict maximum of the other pixels of its window
            win = c.heat[0, max(y - r, 0):y + r + 1, max(x - r, 0):x + r + 1]
            assert int((win >= c.heat[0, y, x]).sum()) == 1
        assert sorted(min(y, x, Hh - 1 - y, Wh - 1 - x) for _, y, x in c.kept) == [1, 1, 1, 1]
    if family == "tiny":
        assert r == 8 and Hh == 8 and Wh in (8, 264)
    if family == "threshold":
        t = np.float32(c.thr)
        vals = c.heat.flatten().numpy()
        assert t in vals and np.nextafter(t, np.float32(np.inf)) in vals and np.nextafter(t, np.float32(-np.inf)) in vals
        if name == "threshold-0.1":                                  # the case that separates float32(thr) from the Python double
            assert float(t) > c.thr and bool(R.pixel_decisions(c.heat.double(), c.k, c.border, c.thr)[0][0, 4, 4])
        if name == "threshold-negative":
            z = c.heat[0, 4, [4, 10]]
            assert _bits(z).tolist() == [0, -2 ** 31] and n_cand[1] == 2
    if family == "borders" and "all" not in name:
        bd = c.border
        inner = lambda v, size: bd <= v < size - bd
        assert sorted(x for _, y, x in c.dropped if inner(y, Hh)) == [bd - 1, Wh - bd] and sorted(y for _, y, x in c.dropped if inner(x, Wh)) == [bd - 1, Hh - bd]
        assert {bd, Wh - bd - 1} <= {x for _, y, x in c.kept} and {bd, Hh - bd - 1} <= {y for _, y, x in c.kept}
        assert len(c.kept) == 4 and len(c.dropped) == 4
    if family in ("lattice", "topk_ties", "min_stack"):
        assert c.k == 3 and c.border == 0 and c.n_cand is not None
        sites = [y * Wh + x for y, x in cases.lattice_sites(Hh, Wh)]
        for b, s in enumerate(sel):
            cand = torch.nonzero(keep[b].flatten()).flatten().tolist()
            assert cand == sites[:len(cand)]                         # the lattice, filled in raster order
    if family == "lattice":
        vals = c.heat[c.heat != 0]
        assert len(vals.unique()) == (1 if "equal" in name else len(vals))
        if name.endswith("-cut"):
            assert not bool((sel[0]["idx"][1:] > sel[0]["idx"][:-1]).all())          # the descending order is not the raster order
    if family == "topk_ties":
        idx = sel[0]["idx"].tolist()
        if "interleaved" in name:
            cand = torch.nonzero(keep[0].flatten()).flatten().tolist()
            pos = [cand.index(i) for i in idx]                       # position in the candidate list = thread of sp_select_kernel
            cut_value = float(sel[0]["score"][-1])
            run = [p for p, i in zip(pos, idx) if float(c.heat[0].flatten()[i]) == cut_value]
            left_out = [p for p, i in enumerate(cand) if float(c.heat[0].flatten()[i]) == cut_value and i not in idx]
            assert min(run) < cases.TILE <= max(run) and left_out and min(left_out) > max(run)
        else:
            assert idx == sites[:m]
    if family == "min_stack":
        assert B > 1
        for s in sel:
            asc = bool((s["idx"][1:] > s["idx"][:-1]).all())
            assert asc == (s["order"] == "raster") or m < 2


def test_tile_boundary_counts():
    counts = sorted({c.n_cand[0] for n, c in cases.CASES.items() if n.startswith("lattice")})
    assert counts[:3] == [256, 257, 512] and counts[3] > 1024
    assert {c.max_kpts for n, c in cases.CASES.items() if n.startswith("topk_ties-301")} == {1, 255, 256, 257, 300, 301, 302, 0}
    assert sorted((c.heat.shape[2], c.k) for n, c in cases.CASES.items() if n.startswith("seam")) == \
        [(w, k) for w in (264, 512, 520) for k in (3, 9, 17)]
    assert {c.border for n, c in cases.CASES.items() if n.startswith("borders-b")} == {1, 4, 8}


# ---------------------------------------------------------------- a second implementation, loops over pixels
def _keep_at(h, y, x, k, border, thr):
    """one pixel: the window with clamped coordinates, centre left out; then threshold, non-zero, borders"""
    H, W = h.shape
    r = (k - 1) // 2
    best = -np.inf
    for yy in range(y - r, y + r + 1):
        row = h[min(max(yy, 0), H - 1)]
        for xx in range(x - r, x + r + 1):
            if yy == y and xx == x:
                continue
            best = max(best, row[min(max(xx, 0), W - 1)])
    v = h[y, x]
    return bool(v > best and v > thr and v != 0 and border <= x < W - border and border <= y < H - border)


def _stack_loops(cands, max_kpts):
    """cands: per image [(raster index, score)] in raster order -> per image the kept indices in output order"""
    limit = [len(c) if (max_kpts == -1 or max_kpts >= len(c)) else max_kpts for c in cands]
    out = []
    for c, lim in zip(cands, limit):
        if len(set(limit)) == 1 and lim == len(c):
            out.append([i for i, _ in c])
        else:
            ranked = sorted(c, key=lambda t: (-t[1], t[0]))
            out.append([i for i, _ in ranked[:lim if len(set(limit)) == 1 else min(limit)]])
    return out


@pytest.mark.parametrize("name", NAMES)
def test_loops_agree_with_restatement(name):
    c = cases.CASES[name]
    B, Hh, Wh = c.heat.shape
    r = (c.k - 1) // 2
    h = c.heat.double().numpy()
    thr = cases.thr32(c.thr)
    keep, _ = R.pixel_decisions(c.heat.double(), c.k, c.border, thr)
    if Hh * Wh * c.k * c.k <= 400_000:
        pixels = [(y, x) for y in range(Hh) for x in range(Wh)]
    else:                                                           # larger: the columns around every seam and edge, the named pixels, a seeded sample
        cols = {x for x0 in range(0, Wh + 1, cases.SEG) for x in range(x0 - r - 1, x0 + r + 1) if 0 <= x < Wh} | set(range(Wh - r - 1, Wh))
        rs = np.random.RandomState(7)
        pixels = [(y, x) for y in range(0, Hh, 5) for x in sorted(cols)] + [(y, x) for _, y, x in c.kept + c.dropped]
        pixels += [(int(i) // Wh, int(i) % Wh) for i in rs.choice(Hh * Wh, 300, replace=False)]
    for b in range(B):
        for y, x in pixels:
            assert _keep_at(h[b], y, x, c.k, c.border, thr) == bool(keep[b, y, x]), (name, b, y, x)
    cands = [[(int(i), float(h[b].flatten()[i])) for i in np.nonzero(keep[b].flatten().numpy())[0]] for b in range(B)]
    mine = _stack_loops(cands, c.max_kpts)
    for b, s in enumerate(_select(c)):
        assert s["idx"].tolist() == mine[b], (name, b)
        assert torch.equal(s["score"], c.heat[b].double().flatten()[s["idx"]])


# ---------------------------------------------------------------- the reference's chain of library calls, where kornia is installed
def _without_borders(kp, sc, border, H, W):
    ok = (kp[:, 0] >= border) & (kp[:, 0] < H - border) & (kp[:, 1] >= border) & (kp[:, 1] < W - border)
    return kp[ok], sc[ok]


def _best_k(kp, sc, k):
    if k == -1 or k >= len(kp):
        return kp, sc
    top = torch.topk(sc, k, dim=0)
    return kp[top.indices], top.values


def _stack_to_min(kps, scs):
    n = min(len(k) for k in kps)
    if all(len(k) == n for k in kps):
        return kps, scs
    keep = [torch.topk(s, n, dim=0).indices for s in scs]
    return [k[i] for k, i in zip(kps, keep)], [s[i] for s, i in zip(scs, keep)]


def test_chain_on_cpu_torch():
    subpix = pytest.importorskip("kornia.geometry.subpix", reason="kornia is not installed: the nms2d chain is not compared")
    for name in NAMES:
        _chain(subpix, name)


def _chain(subpix, name):
    c = cases.CASES[name]
    B, Hh, Wh = c.heat.shape
    nms = subpix.nms2d(c.heat.unsqueeze(1), kernel_size=(c.k, c.k)).squeeze(1)
    kps = [torch.nonzero(F.threshold(s, c.thr, 0.0)) for s in nms]
    scs = [s[tuple(k.t())] for s, k in zip(nms, kps)]
    pairs = [_best_k(*_without_borders(k, s, c.border, Hh, Wh), c.max_kpts) for k, s in zip(kps, scs)]
    kps, scs = _stack_to_min([p[0] for p in pairs], [p[1] for p in pairs])
    for b, s in enumerate(_select(c)):
        idx = kps[b][:, 0] * Wh + kps[b][:, 1]
        assert len(idx) == len(s["idx"]), (name, b)
        if s["order"] == "raster":
            assert torch.equal(idx, s["idx"]) and torch.equal(scs[b].double(), s["score"])
            continue
        # torch.topk leaves the order of equal scores open: the score sequence is fixed, and the set wherever the cut is not in a tie
        assert torch.equal(scs[b].double(), s["score"]), (name, b)
        if len(s["idx"]) and float((s["cut_margin"] == 0).sum()) == 1:
            assert set(idx.tolist()) == set(s["idx"].tolist()), (name, b)
        else:
            strict = s["score"] > (s["score"][-1] if len(s["idx"]) else 0)
            assert set(s["idx"][strict].tolist()) <= set(idx.tolist())
            assert set(idx.tolist()) <= set(s["cand_idx"].tolist())


# ---------------------------------------------------------------- describe inputs
@pytest.mark.parametrize("Hc,Wc", cases.DESCRIBE_SHAPES)
def test_describe_inputs(Hc, Wc):
    pixels = cases.describe_pixels(Hc, Wc)
    Hh, Wh = Hc * 8, Wc * 8
    assert len(set(pixels)) == len(pixels) and all(0 <= p < Hh * Wh for p in pixels)
    stats = cases.tap_stats(Hc, Wc, pixels)
    print(f"describe {Hc} x {Wc}: {len(pixels)} pixels, taps outside the map {stats}")
    for side in ("left", "right", "top", "bottom", "top-left", "top-right", "bottom-left", "bottom-right"):
        assert stats[side] > 0, (Hc, Wc, side)
    assert (stats["inside"] > 0) == (Hc > 1 and Wc > 1)             # with one row or column of cells a tap is always outside
    if Hh * Wh <= 512:
        assert sorted(pixels) == list(range(Hh * Wh))
    else:
        have = set(pixels)
        assert {0, Wh - 1, (Hh - 1) * Wh, Hh * Wh - 1} <= have
        assert {(Hh - 1) * Wh + x for x in range(Wh)} <= have and {y * Wh + Wh - 1 for y in range(Hh)} <= have
        assert any(all(y * Wh + x in have for c in range(1, Wc) for x in (8 * c - 1, 8 * c)) for y in range(Hh - 1))
        assert Hc == 1 or any(all(y * Wh + x in have for c in range(1, Hc) for y in (8 * c - 1, 8 * c)) for x in range(Wh - 1))
    # every run of the GPU test is covered, the list as a whole too
    runs = cases.describe_runs(Hc, Wc)
    assert [n for n, _ in runs][:7] == cases.DESCRIBE_N
    assert set().union(*[set(cases.take(pixels, first, n)) for n, first in runs]) == set(pixels)
    # the sample position is never on a cell centre line: the floor of fp32 arithmetic is the floor of float64
    ix, iy, _, _ = cases.taps(Hc, Wc, pixels)
    frac = np.minimum(np.abs(ix - np.round(ix)), np.abs(iy - np.round(iy)))
    assert frac.min() > 1e-4, frac.min()
    # zero variant: exactly the predicted pixels come out as the zero vector, some of them with all four taps inside the map
    xy = torch.tensor([[p % Wh, p // Wh] for p in pixels], dtype=torch.float64)
    for zero in (False, True):
        d = cases.describe_maps(Hc, Wc, 2, zero)
        assert zero or bool(((d.double().norm(dim=-1) - 1).abs() < 1e-6).all())
        assert not torch.equal(d[0], d[1]) or (zero and Hc * Wc == 1)
        out = R.describe(d[0], xy)
        assert bool(torch.isfinite(out).all())
        pred = cases.all_taps_zero(Hc, Wc, pixels, zero)
        assert np.array_equal((out == 0).all(1).numpy(), pred)
        assert bool(((out.norm(dim=1) - 1).abs() < 1e-12)[torch.from_numpy(~pred)].all())
    only_cells = cases.all_taps_zero(Hc, Wc, pixels, True) & ~cases.all_taps_zero(Hc, Wc, pixels, False)
    _, _, x0, y0 = cases.taps(Hc, Wc, pixels)
    inside = (x0 >= 0) & (x0 + 1 < Wc) & (y0 >= 0) & (y0 + 1 < Hc)
    print(f"describe {Hc} x {Wc}: zero output for {int(pred.sum())} pixels, {int(only_cells.sum())} through cleared cells, "
          f"{int((only_cells & inside).sum())} with four taps inside")
    assert only_cells.sum() > 0 and ((only_cells & inside).sum() > 0) == (Hc > 1 and Wc > 1)
