"""The stages of the SIFT extractor (csrc/sift.hip) on crafted inputs (tests/sift_cases.py; tests/test_sift_cases_cpu.py proves on the
CPU that each case reaches the edge it names), each stage fed test-built buffers and held to the float64 restatement (tests/sift_ref.py).

Detect: counts and det_i rows equal to sift_ref.detect in order, det_f within 1e-9 relative (test_detect's bound: exp2 is the only
inexact step), rows at and after the count still zero; every case runs three times on one workspace -- filled with 0xFF, as the first
call left it, zeroed -- and the three answers are bit-identical.  Orient: one oriented keypoint per reference peak in the reference's
order, angles within 1e-3 degrees (test_orient's bound), every other column equal, no exemption (the margins are proved on the CPU).
Describe: the zero cases exactly zero, the clamp and border cases within 1e-4 on the float path (test_describe's bound); gradients
exactly along the keypoint's axes, which made the float path return NaN before this file (see test_describe_float_path).  Select: the
kept indices exactly those of sift_ref.select.

Overflow cases run with B = 2, the overflowing image in slot 0 and a sparse image in slot 1, so that a missed guard lands in image
1's rows of the same allocation, where the test sees it, and never past the end of a buffer.

What the file found: sift_describe_kernel returned NaN on the float RootSIFT path for a keypoint whose gradients lie exactly along
its own axes (a negative trilinear weight of -1e-7 from a contracted multiply-subtract; fixed in sift.hip, pinned by
test_describe_float_path[axes-*] and test_orient_overflow_and_describe_after_it).

Single-line changes of sift.hip tried on a scratch copy, each built as a library of its own and run on an MI355X against this file
(75 tests) and tests/test_gpu_sift.py (18 tests); the unchanged source passes all 93.  What failed here, and in brackets what
failed there:
  1  extremum test `>=` -> `>` (`<=` -> `<`)  test_detect_exact[moved-mixed, moved-to-layer3, moved-one-column, fifth-step, sixth-step, big,
     (the centre sample left out of the       checkerboard-16x16, checkerboard-24x40], test_detect_exactly_full,
     loop, which compares it with itself:     test_orient_after_overflowed_detect                                                    [none]
     the literal change keeps nothing)        (tie-pair and plateau do not tell: their candidates are dropped with or without the tie)
  2  `v != 0.f` removed                       test_detect_exact[zero-extrema]                                                        [none]
  3  `< 0.5` -> `<= 0.5`                      test_detect_exact[tie-pair, big]                                                       [none]
  4  `c >= w - SIFT_BORDER` -> `>`            test_detect_exact[moved-onto-border]                                                   [none]
  5  `l > SIFT_S` -> `>=`                     test_detect_exact[moved-mixed, moved-to-layer3, fifth-step, sixth-step]
                                                                         [test_detect[64x64, 97x131, 3x120x160], test_homography_pair]
  6  SIFT_MAX_STEPS 5 -> 6                    test_detect_exact[sixth-step]                                 [test_detect[97x131, 3x120x160]]
  7  `ph[k - 1] < v` -> `<=`                  test_orient_exact[two-peaks-tie, four-tie, three, wrap-to-zero, wrap-negative,
                                              no-gradient-between], test_orient_overflow_and_describe_after_it                       [none]
  8  the `bn < 0` wrap removed                test_orient_exact[wrap-to-zero, wrap-negative], test_orient_wrap_to_zero_reports_zero  [none]
  9  `off >= cap` -> `> cap`                  test_detect_exact[checkerboard-16x16, checkerboard-24x40],
                                              test_orient_after_overflowed_detect                                                    [none]
                                              (at 16 x 16 image 0 passes cap in octave 1, a launch after the one that wrote image 1's
                                              row 0, so the stray write always shows; at 24 x 40 both happen in the octave 0 launch and
                                              the order of the workgroups decides: it failed in this run, only 16 x 16 is certain to)
 10  `tot > capn` -> `>=`                     test_select_exact[clusters-exactly-capn]                                               [none]
     (removing a guard outright -- `off >= cap`, `off + k >= g.cap2`, `out + cnt < capn` -- writes past a per-image buffer: not run)
"""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sift_cases as C  # noqa: E402
import sift_ref as R  # noqa: E402

from openglue_amd.sift import SIFT, geometry  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
DETECT = {c.name: c for c in C.detect_cases()}
ORIENT = {c.name: c for c in C.orient_cases()}
DESCRIBE = {c.name: c for c in C.describe_cases()}
SELECT = {c.name: c for c in C.select_cases()}
DET_TOL = 1e-9               # relative, test_gpu_sift.test_detect
ANGLE_TOL = 1e-3             # degrees, test_gpu_sift.test_orient
DESC_TOL = 1e-4              # test_gpu_sift.test_describe


def _f64(vols):
    return [v.astype(np.float64) for v in vols]


def _flat(images):
    """[image][octave] arrays -> the packed [B, floats] buffer the stages take"""
    return torch.from_numpy(np.stack([np.concatenate([v.reshape(-1) for v in vols]) for vols in images]).astype(np.float32)).to(DEV)


def _counts(B, **at):
    c = torch.zeros(4 * B + 1, dtype=torch.int32)
    for k, v in at.items():
        c[int(k[1:])] = v
    return c.to(DEV)


# ---------------------------------------------------------------- detect
@functools.lru_cache(maxsize=None)
def _detect_reference(name):
    return [R.detect(_f64(dog)) for dog in DETECT[name].dog]


def _run_detect(net, dog, H, W, ws):
    counts = net.new_counts(dog.shape[0], DEV)
    det_i, det_f = net.detect(dog, H, W, counts, ws)
    torch.cuda.synchronize()
    return counts.cpu(), det_i.cpu(), det_f.cpu()


def _check_detect(name, out, B, cap):
    counts, det_i, det_f = (t.numpy() for t in out)
    for b, (ki, kf) in enumerate(_detect_reference(name)):
        assert counts[b] == len(ki), (name, b, counts.tolist(), len(ki))
        n = min(len(ki), cap)
        assert np.array_equal(det_i[b, :n], ki[:n]), (name, b)
        assert (np.abs(det_f[b, :n] - kf[:n]) <= DET_TOL * np.abs(kf[:n])).all(), (name, b)
        assert not det_i[b, n:].any() and not det_f[b, n:].any(), (name, b)
    assert not counts[B:].any()


@pytest.mark.parametrize("name", list(DETECT))
def test_detect_exact(name):
    c = DETECT[name]
    B, net, geom = len(c.dog), SIFT(), geometry(c.H, c.W)
    assert (geom.cap, geom.cap2) == C.capacities(c.H, c.W)[:2] and geom.octaves == R.octave_sizes(c.H, c.W)
    dog = _flat(c.dog)
    ws = net.workspace(B, c.H, c.W, DEV)
    ws.fill_(0xFF)
    first = _run_detect(net, dog, c.H, c.W, ws)
    _check_detect(name, first, B, geom.cap)
    again = _run_detect(net, dog, c.H, c.W, ws)                 # on what the first call left in the workspace
    ws.zero_()
    zeroed = _run_detect(net, dog, c.H, c.W, ws)
    for other in (again, zeroed):
        assert all(torch.equal(a, b) for a, b in zip(first[:2], other[:2])), name
        assert torch.equal(first[2].view(torch.int64), other[2].view(torch.int64)), name
    over = [len(ki) > geom.cap for ki, _ in _detect_reference(name)]
    if any(over):
        assert over[0] and not over[-1]                         # never the last image of the batch
        with pytest.raises(RuntimeError, match="keypoints"):
            SIFT.check_counts(first[0], B, geom)
    else:
        SIFT.check_counts(first[0], B, geom)


def test_detect_exactly_full():
    """cap keypoints exactly: nothing is cut, nothing raises; with the sparse image in front or behind"""
    H = W = 16
    net, geom = SIFT(), geometry(H, W)
    full, sparse = C.checkerboard_full(), C.sparse_dog(H, W)
    ref = {"full": R.detect(_f64(full)), "sparse": R.detect(_f64(sparse))}
    assert len(ref["full"][0]) == geom.cap
    for order in (("full", "sparse"), ("sparse", "full")):
        vols = {"full": full, "sparse": sparse}
        ws = net.workspace(2, H, W, DEV)
        counts, det_i, det_f = (t.numpy() for t in _run_detect(net, _flat([vols[k] for k in order]), H, W, ws))
        assert SIFT.check_counts(torch.from_numpy(counts), 2, geom) == 0
        for b, k in enumerate(order):
            ki, kf = ref[k]
            assert counts[b] == len(ki) and np.array_equal(det_i[b, :len(ki)], ki) and not det_i[b, len(ki):].any()
            assert (np.abs(det_f[b, :len(ki)] - kf) <= DET_TOL * np.abs(kf)).all()


# ---------------------------------------------------------------- orient
def _det_buffers(kis, kfs, cap):
    B = len(kis)
    det_i = torch.zeros(B, cap, 4, dtype=torch.int32)
    det_f = torch.zeros(B, cap, 4, dtype=torch.float64)
    for b, (ki, kf) in enumerate(zip(kis, kfs)):
        det_i[b, :len(ki)] = torch.from_numpy(np.asarray(ki, dtype=np.int32))
        det_f[b, :len(ki)] = torch.from_numpy(np.asarray(kf, dtype=np.float64))
    return det_i.to(DEV), det_f.to(DEV)


def _run_orient(H, W, gauss, det_i, det_f, counts, upright=False):
    net = SIFT(upright=upright)
    ws = net.workspace(det_i.shape[0], H, W, DEV)
    ws.fill_(0xFF)
    ori_i, ori_f = net.orient(gauss, H, W, det_i, det_f, counts, ws)
    torch.cuda.synchronize()
    return counts.cpu().numpy(), ori_i.cpu().numpy(), ori_f.cpu().numpy()


def _check_orient(tag, gi, gf, count, oi, of, cap2):
    assert count == len(oi), (tag, int(count), len(oi))
    m = min(len(oi), cap2)
    assert np.array_equal(gi[:m], oi[:m]), tag
    dang = np.abs((gf[:m, 3].astype(np.float64) - of[:m, 3] + 180.0) % 360.0 - 180.0)
    assert (dang <= ANGLE_TOL).all(), (tag, float(dang.max()) if m else 0.0)
    assert np.array_equal(gf[:m][:, [0, 1, 2, 4]], of[:m][:, [0, 1, 2, 4]]), tag
    assert not gi[m:].any() and not gf[m:].any(), tag
    assert m == 0 or ((gf[:m, 3] >= 0.0) & (gf[:m, 3] < 360.0)).all(), tag


@pytest.mark.parametrize("upright", [False, True])
@pytest.mark.parametrize("name", list(ORIENT))
def test_orient_exact(name, upright):
    c = ORIENT[name]
    geom = geometry(c.H, c.W)
    det_i, det_f = _det_buffers([c.ki], [c.kf], geom.cap)
    counts, gi, gf = _run_orient(c.H, c.W, _flat([c.gauss]), det_i, det_f, _counts(1, c0=len(c.ki)), upright)
    oi, of, _ = R.orient(_f64(c.gauss), c.ki, c.kf, upright)
    if not upright and c.peaks is not None:
        assert np.bincount(oi[:, 5], minlength=len(c.ki)).tolist() == c.peaks
    _check_orient((name, upright), gi[0], gf[0], counts[1], oi, of, geom.cap2)
    assert counts[0] == len(c.ki) and not counts[2:].any()


def test_orient_wrap_to_zero_reports_zero():
    """the angle that rounds to 360.f in float32 comes out as exactly 0, not as 360"""
    c = ORIENT["wrap-to-zero"]
    geom = geometry(c.H, c.W)
    det_i, det_f = _det_buffers([c.ki], [c.kf], geom.cap)
    _, _, gf = _run_orient(c.H, c.W, _flat([c.gauss]), det_i, det_f, _counts(1, c0=1))
    assert sorted(gf[0, :4, 3].tolist()) == [0.0, 90.0, 180.0, 270.0]


# ---------------------------------------------------------------- describe
def _ori_buffers(ois, ofs, cap2):
    B = len(ois)
    ori_i = torch.zeros(B, cap2, 6, dtype=torch.int32)
    ori_f = torch.zeros(B, cap2, 5, dtype=torch.float32)
    for b, (oi, of) in enumerate(zip(ois, ofs)):
        ori_i[b, :len(oi), :np.asarray(oi).shape[1]] = torch.from_numpy(np.asarray(oi, dtype=np.int32))
        ori_f[b, :len(of)] = torch.from_numpy(np.asarray(of, dtype=np.float32))
    return ori_i.to(DEV), ori_f.to(DEV)


def _run_describe(c, quantize, rootsift, normalize):
    geom = geometry(c.H, c.W)
    ori_i, ori_f = _ori_buffers([c.oi], [c.of], geom.cap2)
    net = SIFT(quantize=quantize, rootsift=rootsift)
    desc = net.describe(_flat([c.gauss]), c.H, c.W, ori_i, ori_f, _counts(1, c1=len(c.oi)), normalize=normalize)
    torch.cuda.synchronize()
    return desc[0, :len(c.oi)].cpu().numpy()


@pytest.mark.parametrize("quantize", [True, False])
@pytest.mark.parametrize("rootsift", [1, 0, -1])
def test_describe_zero(quantize, rootsift):
    d = _run_describe(DESCRIBE["constant"], quantize, rootsift == 1, rootsift >= 0)
    assert d.shape == (3, 128) and not d.any()


@pytest.mark.parametrize("name", [n for n in DESCRIBE if n != "constant"])
def test_describe_float_path(name):
    """The float path against the restatement within test_describe's 1e-4, before the RootSIFT step and after it.  The axes cases
    have bins that are exactly 0 in float64 and 1e-8 of the total on the GPU (atan2f(0, -x) in degrees is 180 to one ulp, 1.5e-5
    degrees, which leaks 3e-7 of a sample into the next orientation bin); the RootSIFT square root turns 1e-8 into 1e-4.  That is
    the square root's slope at 0, not an error of the kernel, so after RootSIFT those cases are compared as squares -- the
    L1-normalised histogram, in which the leak is linear -- under the same bound, and every value must be finite and >= 0."""
    c = DESCRIBE[name]
    g = _f64(c.gauss)
    raw = np.stack([R.finish_descriptor(R.raw_descriptor(g, c.oi[k], c.of[k, 2], c.of[k, 3]), False) for k in range(len(c.oi))])
    d = _run_describe(c, False, True, False)
    assert np.isfinite(d).all() and (d >= 0).all()
    assert float(np.abs(d - raw).max()) <= DESC_TOL
    ref = R.describe(g, c.oi, c.of, quantize=False, rootsift=True)
    d = _run_describe(c, False, True, True).astype(np.float64)
    assert np.isfinite(d).all() and (d >= 0).all()
    err, err2 = float(np.abs(d - ref).max()), float(np.abs(d * d - ref * ref).max())
    print(f"sift describe {name}: RootSIFT max |d| {err:.3e}, of the squares {err2:.3e}")
    assert (err2 if name.startswith("axes-") else err) <= DESC_TOL
    assert (ref[np.abs(d - ref) > DESC_TOL] == 0.0).all()             # only exactly empty bins miss the plain bound


# ---------------------------------------------------------------- select
def _run_select(c):
    B = len(c.of)
    net, geom = SIFT(max_keypoints=c.max_kpts, nms_diameter=c.diameter), geometry(c.H, c.W)
    ori_i, ori_f = _ori_buffers(c.keys, c.of, geom.cap2)
    counts = _counts(B, **{f"c{B + b}": len(of) for b, of in enumerate(c.of)})
    ws = net.workspace(B, c.H, c.W, DEV)
    ws.fill_(0xFF)
    sel = net.select(c.H, c.W, ori_i, ori_f, counts, ws)
    torch.cuda.synchronize()
    return net, geom, counts.cpu(), sel.cpu().numpy(), ori_f


@pytest.mark.parametrize("name", list(SELECT))
def test_select_exact(name):
    c = SELECT[name]
    B = len(c.of)
    net, geom, counts, sel, ori_f = _run_select(c)
    refs = [R.select(of[:, :2], of[:, 4], R.sort_keys(k), c.diameter, c.max_kpts) for of, k in zip(c.of, c.keys)]
    cn = counts.numpy()
    over = [c.entries is not None and c.entries[b] > C.NBR_AVG * geom.cap2 for b in range(B)]
    for b in range(B):
        if c.entries is not None:
            assert cn[3 * B + b] == c.entries[b], (name, b, cn.tolist())
        if over[b]:
            assert cn[2 * B + b] == 0, (name, b, cn.tolist())           # reported, and nothing is kept
        else:
            assert cn[2 * B + b] == len(refs[b]), (name, b, cn.tolist())
            assert np.array_equal(sel[b, :len(refs[b])], refs[b]), (name, b)
    assert cn[4 * B] == min(cn[2 * B:3 * B])
    if any(over):
        assert c.overflow and over[0] and not over[-1]
        with pytest.raises(RuntimeError, match="NMS neighbour entries"):
            net.check_counts(counts, B, geom)
    else:
        m = net.check_counts(counts, B, geom)
        assert m == min(len(r) for r in refs)
        lafs, scores, desc = net.gather(c.H, c.W, m, torch.from_numpy(sel).to(DEV), ori_f, torch.zeros(B, geom.cap2, 128, device=DEV))
        torch.cuda.synchronize()
        assert lafs.shape == (B, m, 2, 3) and scores.shape == (B, m) and desc.shape == (B, m, 128)
        for b in range(B):
            assert np.array_equal(scores[b].cpu().numpy(), c.of[b][refs[b][:m], 4])


# ---------------------------------------------------------------- overflow chains
def test_orient_after_overflowed_detect():
    """the 16 x 16 checkerboard (1040 keypoints, cap 1024) through detect and orient on a plane of constant gradient: orient uses the
    first cap keypoints of image 0 and leaves image 1 right"""
    c = DETECT["checkerboard-16x16"]
    H, W, B = c.H, c.W, 2
    net, geom = SIFT(), geometry(c.H, c.W)
    ws = net.workspace(B, H, W, DEV)
    counts = net.new_counts(B, DEV)
    det_i, det_f = net.detect(_flat(c.dog), H, W, counts, ws)
    planes = [np.stack([C.ramp(h, w)] * 6).astype(np.float32) for h, w in geom.octaves]
    gauss = _flat([planes, planes])
    ori_i, ori_f = net.orient(gauss, H, W, det_i, det_f, counts, ws)
    torch.cuda.synchronize()
    cn, gi, gf = counts.cpu().numpy(), ori_i.cpu().numpy(), ori_f.cpu().numpy()
    assert cn[:2].tolist() == [1040, 4]
    for b, (ki, kf) in enumerate(_detect_reference(c.name)):
        oi, of, near = R.orient(_f64(planes), ki[:geom.cap], kf[:geom.cap])
        assert near.min() >= 1e-3 and len(oi) == min(len(ki), geom.cap)
        _check_orient(("after-detect", b), gi[b], gf[b], cn[B + b], oi, of, geom.cap2)
    with pytest.raises(RuntimeError, match="image 0 has 1040 keypoints"):
        net.check_counts(counts.cpu(), B, geom)


def test_orient_overflow_and_describe_after_it():
    """cap copies of a two-peak keypoint: 2048 oriented keypoints against cap2 = 1280.  The true count is reported, the first cap2 rows
    are right, image 1 is intact; describe then writes cap2 rows for image 0 and image 1's rows are right"""
    H, W, gauss, kis, kfs = C.two_peak_overflow()
    B, geom = 2, geometry(H, W)
    det_i, det_f = _det_buffers(kis, kfs, geom.cap)
    g = _flat(gauss)
    counts = _counts(B, c0=len(kis[0]), c1=len(kis[1]))
    net = SIFT(quantize=False)
    ws = net.workspace(B, H, W, DEV)
    ws.fill_(0xFF)
    ori_i, ori_f = net.orient(g, H, W, det_i, det_f, counts, ws)
    desc = net.describe(g, H, W, ori_i, ori_f, counts)
    torch.cuda.synchronize()
    cn, gi, gf, d = counts.cpu().numpy(), ori_i.cpu().numpy(), ori_f.cpu().numpy(), desc.cpu().numpy()
    refs = [R.orient(_f64(gauss[b]), kis[b], kfs[b]) for b in range(B)]
    assert cn[B] == 2048 > geom.cap2 and cn[B + 1] == 4
    for b in range(B):
        _check_orient(("orient-overflow", b), gi[b], gf[b], cn[B + b], refs[b][0], refs[b][1], geom.cap2)
    with pytest.raises(RuntimeError, match="image 0 has 2048 oriented keypoints"):
        net.check_counts(counts.cpu(), B, geom)
    # describe: image 0's cap2 rows are the two descriptors of the one keypoint, alternating; image 1's four rows
    ref0 = R.describe(_f64(gauss[0]), refs[0][0][:2], refs[0][1][:2], quantize=False, rootsift=True)
    def sq(a, r):             # axis-aligned gradients: see test_describe_float_path; only exactly empty bins may miss the plain bound
        assert (r[np.abs(a - r) > DESC_TOL] == 0.0).all()
        return float(np.abs(a.astype(np.float64) ** 2 - r * r).max())
    assert np.isfinite(d[0, :geom.cap2]).all() and sq(d[0, :2], ref0) <= DESC_TOL
    assert np.array_equal(d[0, 2:geom.cap2], np.tile(d[0, :2], (geom.cap2 // 2 - 1, 1)))
    ref1 = R.describe(_f64(gauss[1]), refs[1][0], refs[1][1], quantize=False, rootsift=True)
    assert np.isfinite(d[1, :4]).all() and sq(d[1, :4], ref1) <= DESC_TOL


def _dense_batch():
    """image 0: bright dots every 10 pixels of a 96 x 96 image (the restatement finds 226 keypoints with 959 orientations), image 1
    flat.  With an NMS radius that spans the image every pair is a neighbour entry: 459361 against the 184320 there is room for."""
    img = torch.full((2, 1, 96, 96), 0.5)
    img[0] = 0.0
    img[0, 0, 5::10, 5::10] = 1.0
    return img.to(DEV)


def test_forward_raises_on_overflow():
    with pytest.raises(RuntimeError, match="image 0 has [0-9]+ NMS neighbour entries"):
        SIFT(nms_diameter=400.)(_dense_batch())
    lafs, scores, desc = SIFT(nms_diameter=9.)(_dense_batch())          # the same batch fits at the default radius: image 1 keeps 0
    assert scores.shape == (2, 0) and lafs.shape == (2, 0, 2, 3) and desc.shape == (2, 0, 128)
    lafs, scores, desc = SIFT(nms_diameter=9.)(_dense_batch()[:1])
    assert scores.shape[1] > 100


def test_dog_affnet_hardnet_detect_raises_on_overflow():
    from openglue_amd.affnet_hardnet import DoGAffNetHardNet
    with pytest.raises(RuntimeError, match="image 0 has [0-9]+ NMS neighbour entries"):
        DoGAffNetHardNet(nms_diameter=400.).detect(_dense_batch())
