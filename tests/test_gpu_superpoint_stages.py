"""The detect and describe stages of SuperPoint inference (csrc/superpoint.hip: sp_nms_kernel, sp_scan_kernel, sp_compact_kernel,
sp_select_kernel, sp_describe_kernel) on crafted inputs (tests/superpoint_detect_cases.py; tests/test_superpoint_detect_cases_cpu.py
proves on the CPU that each case reaches the edge it names).

Detect: SuperPointNet.detect on the crafted fp32 heatmap against superpoint_ref.select on the same values in float64.  The selection is a
pure comparison of fp32 values, so the comparison is exact: candidate counts, kept count, every index in output order, every score bit for
bit.  No exemption, no tolerance, no parity_note.  Every case runs three times on one workspace -- filled with 0xFF, as the first call
left it, zeroed -- and must give the same answer.

Describe: SuperPointNet.describe on test-built selection buffers against superpoint_ref.describe in float64, bound DESC_TOL = 1e-5 of
tests/test_gpu_superpoint.py.  Measured on an MI355X, worst over all shapes, batch sizes and both variants: max |d| 1.301e-06 for the
kernel, 1.306e-06 for fp32 ATen (grid_sample + F.normalize) on the CPU on the same inputs, both at 4 x 65 cells (1 x 1: 1.6e-08 / 6.0e-08,
2 x 3: 4.6e-08 / 1.2e-07, 1 x 33: 6.7e-07 / 6.7e-07); the error is that of the fp32 sample coordinate, which grows with the map's width.
A descriptor none of whose taps is non-zero comes out as exactly the zero vector.

Single-line changes of superpoint.hip tried on a scratch copy: what failed here, and in brackets what failed of the 20 tests of the
whole-network file tests/test_gpu_superpoint.py (random weights, near-tie exemptions):
  1  sp_nms_kernel `v > mx` -> `v >= mx`              test_detect_exact[seam-*, plateau-*, edge_replicate-*, tiny-8x8-k17-pair, tiny-8x264-k17,
                                                      threshold-negative], test_detect_workspace_offset[seam-*]           [1: 125 x 171, border 0]
  2  halo column clamped to x0 instead of 0           test_detect_exact[seam-* (all nine), tiny-8x264-k17], test_detect_workspace_offset[seam-*]  [none]
  3  `x >= border` -> `x > border`                    test_detect_exact[borders-b1, -b4, -b8, each with and without filler]   [1: nms_kernel 3]
  4  `v != 0.f` removed                               test_detect_exact[threshold-negative]                                   [none]
  5  sp_select_kernel `si[j] < vi` -> `si[j] > vi`    test_detect_exact / test_select_writes_ranks_below_m_only[topk_ties-301-k1, -k255, -k256, -k257,
                                                      -k300, topk_ties-interleaved-*], test_detect_exact[seam-w520-*] (equal peaks at its two seams)
                                                                                                                              [2: 480 x 640, top-k]
  6  `raster = equal && cb == n` -> `equal`           test_detect_exact[lattice-distinct-*-cut, topk_ties-interleaved-*, min_stack-mixed-order],
                                                      test_forward_handover[1, 300]                                           [2: 480 x 640, top-k]
  7  the early return `>= n` -> `> n`                 nothing, here or there: the one more workgroup that then runs when n is a multiple of 256 has no
                                                      live thread and writes nothing; the change costs time and cannot change an output
  8  sp_describe_kernel w_ne and w_sw swapped         test_describe[all but 1 x 1, where the one cell is the only tap and F.normalize cancels its
                                                      weight], test_forward_handover[-1, 1, 300]                              [9]
     (instead of `xx >= Wc` -> `xx > Wc`, which reads past the map's last row with B = 1: not run)
"""
import functools

import pytest
import torch
import torch.nn.functional as F

import superpoint_detect_cases as cases
import superpoint_ref as R
from openglue_amd import _lib
from openglue_amd.superpoint import SuperPointNet
from test_gpu_superpoint import DESC_TOL

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
NAMES = list(cases.CASES)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _net(c):
    return SuperPointNet(max_keypoints=c.max_kpts, nms_kernel=c.k, remove_borders_size=c.border, keypoint_threshold=c.thr).eval()


@functools.lru_cache(maxsize=None)
def _reference(name):
    c = cases.CASES[name]
    return R.select(c.heat.double(), c.k, c.border, cases.thr32(c.thr), c.max_kpts)


def _detect(net, heat, ws):
    counts, sidx, sscore, cap = net.detect(heat, ws)
    torch.cuda.synchronize()
    assert sidx.shape == sscore.shape == (heat.shape[0], cap)
    return counts.cpu(), sidx.cpu(), sscore.cpu()


def _check(name, heat, out, sel):
    """exact: counts, kept count, indices in output order, scores bit for bit"""
    counts, sidx, sscore = out
    B = heat.shape[0]
    m = len(sel[0]["idx"])
    assert counts[:B].tolist() == [s["n_cand"] for s in sel], (name, counts.tolist())
    assert counts[B:].tolist() == [m] * B, (name, counts.tolist(), m)
    assert m <= sidx.shape[1], name
    for b, s in enumerate(sel):
        assert len(s["idx"]) == m
        got = sidx[b, :m].long()
        if not torch.equal(got, s["idx"]):
            at = int(torch.nonzero(got != s["idx"])[0])
            pytest.fail(f"{name} image {b}: output {at} of {m} is pixel {int(got[at])}, float64 selects {int(s['idx'][at])} ({s['order']} order)")
        assert torch.equal(_bits(sscore[b, :m]), _bits(heat[b].flatten()[s["idx"]])), (name, b)
    return m


def _same(a, b, m):
    return torch.equal(a[0], b[0]) and torch.equal(a[1][:, :m], b[1][:, :m]) and torch.equal(_bits(a[2][:, :m]), _bits(b[2][:, :m]))


@pytest.mark.parametrize("name", NAMES)
def test_detect_exact(name):
    c = cases.CASES[name]
    B, Hh, Wh = c.heat.shape
    net = _net(c)
    heat = c.heat.to(DEV)
    ws = net._workspace(B, Hh, Wh, DEV)
    ws.fill_(0xFF)
    first = _detect(net, heat, ws)
    m = _check(name, c.heat, first, _reference(name))
    again = _detect(net, heat, ws)                   # on what the first call left in the workspace
    ws.zero_()
    zeroed = _detect(net, heat, ws)
    assert _same(first, again, m) and _same(first, zeroed, m), name
    assert torch.equal(heat.cpu(), c.heat)           # the input is not written


@pytest.mark.parametrize("name", [n for n in NAMES if n.startswith(("seam", "lattice"))])
def test_detect_workspace_offset(name):
    """the workspace 16 bytes past its natural alignment (the C entry asks for 16, the allocator gives 512)"""
    c = cases.CASES[name]
    B, Hh, Wh = c.heat.shape
    net = _net(c)
    whole = torch.full((net._workspace(B, Hh, Wh, DEV).numel() + 16,), 0xA5, device=DEV, dtype=torch.uint8)
    ws = whole[16:]
    assert ws.data_ptr() % 512 == 16
    _check(name, c.heat, _detect(net, c.heat.to(DEV), ws), _reference(name))


def test_detect_batch_order():
    """the images of a batch in another order: each image's candidates move with it"""
    c = cases.CASES["min_stack-unequal"]
    perm = [2, 0, 1]
    heat = c.heat[perm].contiguous()
    net = _net(c)
    out = _detect(net, heat.to(DEV), net._workspace(*heat.shape, DEV))
    sel = R.select(heat.double(), c.k, c.border, cases.thr32(c.thr), c.max_kpts)
    m = _check("min_stack-unequal permuted", heat, out, sel)
    assert out[0][:3].tolist() == [c.n_cand[p] for p in perm]
    base = _reference("min_stack-unequal")
    for b, p in enumerate(perm):
        assert torch.equal(out[1][b, :m].long(), base[p]["idx"])


@pytest.mark.parametrize("name", [n for n in NAMES if n.startswith(("min_stack", "topk_ties"))])
def test_select_writes_ranks_below_m_only(name):
    """og_superpoint_detect on selection buffers of exactly og_superpoint_capacity columns, pre-filled: columns from the kept count on and
    a guard row behind the last image keep their fill, so sp_select_kernel writes ranks < m and m never exceeds the max_keypoints-sized
    buffer, with unequal counts too"""
    c = cases.CASES[name]
    B, Hh, Wh = c.heat.shape
    cap = _lib.load().og_superpoint_capacity(Hh, Wh, c.max_kpts)
    heat = c.heat.to(DEV)
    counts = torch.full((2 * B + 8,), -7, device=DEV, dtype=torch.int32)
    sidx = torch.full((B + 1, cap), -7, device=DEV, dtype=torch.int32)
    sscore = torch.full((B + 1, cap), -7.0, device=DEV, dtype=torch.float32)
    ws = _net(c)._workspace(B, Hh, Wh, DEV)
    _lib.call("og_superpoint_detect", DEV, B, Hh, Wh, c.k, c.border, float(c.thr), c.max_kpts, heat.data_ptr(), counts.data_ptr(),
              sidx.data_ptr(), sscore.data_ptr(), cap, ws.data_ptr(), _lib.STREAM)
    torch.cuda.synchronize()
    m = _check(name, c.heat, (counts[:2 * B].cpu(), sidx[:B].cpu(), sscore[:B].cpu()), _reference(name))
    assert m <= cap and (c.max_kpts <= 0 or cap <= c.max_kpts)
    assert bool((counts[2 * B:] == -7).all()) and bool((sidx[:B, m:] == -7).all()) and bool((sscore[:B, m:] == -7.0).all())
    assert bool((sidx[B] == -7).all()) and bool((sscore[B] == -7.0).all())


# ---------------------------------------------------------------- describe
def _describe32(desc_nhwc, xy):
    """the reference's chain in fp32 ATen on the CPU, for scale"""
    Hc, Wc, D = desc_nhwc.shape
    p = (xy.to(torch.float32) - 4 + 0.5) / torch.tensor([Wc * 8 - 4.5, Hc * 8 - 4.5], dtype=torch.float32)
    d = F.grid_sample(desc_nhwc.permute(2, 0, 1)[None], (p * 2 - 1).view(1, 1, -1, 2), mode="bilinear", align_corners=False)
    return F.normalize(d.view(D, -1).t(), p=2, dim=1)


def _selection(Hc, Wc, B, n, first, pad=3):
    """sel_idx / sel_score [B, n + pad]: image b holds n pixels of the list from `first` on (another stretch per image); the columns from n on
    hold indices outside the image and NaN scores, which nothing may read"""
    pixels = cases.describe_pixels(Hc, Wc)
    gen = torch.Generator().manual_seed(100 * n + first)
    sidx = torch.empty(B, n + pad, dtype=torch.int32)
    sidx[:, n:] = torch.tensor([Hc * Wc * 64 + 12345, -1, 2 ** 31 - 1][:pad], dtype=torch.int32)
    sscore = torch.rand(B, n + pad, generator=gen)
    sscore[:, n:] = float("nan")
    for b in range(B):
        sidx[b, :n] = torch.tensor(cases.take(pixels, first, n, shift=131 * b), dtype=torch.int32)
    return sidx, sscore


WORST = {"kernel": 0.0, "aten": 0.0}


def _check_describe(tag, desc, sidx, sscore, n, out, zero):
    lafs, scores, descriptors = (t.cpu() for t in out)
    B, Hc, Wc, _ = desc.shape
    Wh = Wc * 8
    assert lafs.shape == (B, n, 2, 3) and scores.shape == (B, n) and descriptors.shape == (B, n, 256)
    worst = aten = 0.0
    for b in range(B):
        idx = sidx[b, :n].long()
        xy = torch.stack([idx % Wh, idx // Wh], 1)
        want = torch.zeros(n, 2, 3)
        want[:, 0, 0], want[:, 1, 1] = 1.0, 1.0
        want[:, :, 2] = xy.float()
        assert torch.equal(_bits(lafs[b]), _bits(want)), (tag, b)
        assert torch.equal(_bits(scores[b]), _bits(sscore[b, :n])), (tag, b)
        assert bool(torch.isfinite(descriptors[b]).all()), (tag, b)
        ref = R.describe(desc[b], xy.double())
        dead = torch.from_numpy(cases.all_taps_zero(Hc, Wc, idx.tolist(), zero))
        assert torch.equal((ref == 0).all(1), dead)
        assert bool((descriptors[b][dead] == 0).all()), (tag, b, "a descriptor with no non-zero tap is exactly the zero vector")
        worst = max(worst, float((descriptors[b].double() - ref).abs().max()))
        aten = max(aten, float((_describe32(desc[b], xy).double() - ref).abs().max()))
        if B > 1 and not bool(dead.all()):           # the other image's map gives something else: the batch offset is the image's own
            other = R.describe(desc[1 - b], xy.double())
            assert float((descriptors[b].double() - other).abs().max()) > 0.01, (tag, b)
    return worst, aten


@pytest.mark.parametrize("zero", [False, True])
@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("Hc,Wc", cases.DESCRIBE_SHAPES)
def test_describe(Hc, Wc, B, zero):
    net = SuperPointNet().eval()
    desc = cases.describe_maps(Hc, Wc, B, zero)
    desc_dev = desc.to(DEV)
    worst = aten = 0.0
    for n, first in cases.describe_runs(Hc, Wc):
        sidx, sscore = _selection(Hc, Wc, B, n, first)
        out = net.describe(n, sidx.to(DEV), sscore.to(DEV), desc_dev)
        torch.cuda.synchronize()
        w, a = _check_describe(f"{Hc}x{Wc} B={B} zero={zero} n={n}", desc, sidx, sscore, n, out, zero)
        worst, aten = max(worst, w), max(aten, a)
    WORST["kernel"], WORST["aten"] = max(WORST["kernel"], worst), max(WORST["aten"], aten)
    print(f"describe {Hc}x{Wc} B={B} zero={zero}: max |d| vs float64 {worst:.3e} (fp32 ATen on the CPU: {aten:.3e}); "
          f"worst so far {WORST['kernel']:.3e} / {WORST['aten']:.3e}")
    assert worst <= DESC_TOL, (worst, aten)


# ---------------------------------------------------------------- detect -> describe as forward() chains them
@pytest.mark.parametrize("max_kpts", [-1, 0, 1, 300])
def test_forward_handover(max_kpts, monkeypatch):
    """net(image) with dense() replaced by crafted tensors: counts[B], the selection buffers and their leading dimension
    (og_superpoint_capacity) go from detect to describe as forward() passes them.  Counts (300, 500): -1 cuts both to 300 in descending
    order, 0 keeps none, 1 the best of each, 300 leaves image 0 in raster order beside image 1 cut."""
    c = cases.CASES["min_stack-unequal-caps"]
    B, Hh, Wh = c.heat.shape
    desc = cases.describe_maps(Hh // 8, Wh // 8, B, False)
    net = SuperPointNet(max_keypoints=max_kpts, nms_kernel=c.k, remove_borders_size=c.border, keypoint_threshold=c.thr).eval()
    heat_dev, desc_dev = c.heat.to(DEV), desc.to(DEV)
    monkeypatch.setattr(net, "dense", lambda image, workspace=None: (heat_dev, desc_dev))
    lafs, scores, descriptors = (t.cpu() for t in net(torch.zeros(B, 1, Hh, Wh, device=DEV)))
    torch.cuda.synchronize()
    sel = R.select(c.heat.double(), c.k, c.border, cases.thr32(c.thr), max_kpts)
    m = {-1: 300, 0: 0, 1: 1, 300: 300}[max_kpts]
    assert [s["order"] for s in sel] == {-1: ["desc", "desc"], 0: ["desc", "desc"], 1: ["desc", "desc"], 300: ["raster", "desc"]}[max_kpts]
    assert lafs.shape == (B, m, 2, 3) and scores.shape == (B, m) and descriptors.shape == (B, m, 256)
    for b, s in enumerate(sel):
        assert len(s["idx"]) == m
        assert torch.equal(lafs[b, :, 1, 2].long() * Wh + lafs[b, :, 0, 2].long(), s["idx"]), (max_kpts, b)
        assert torch.equal(_bits(scores[b]), _bits(c.heat[b].flatten()[s["idx"]]))
        if m:
            xy = torch.stack([s["idx"] % Wh, s["idx"] // Wh], 1).double()
            assert float((descriptors[b].double() - R.describe(desc[b], xy)).abs().max()) <= DESC_TOL
