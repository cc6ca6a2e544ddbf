"""The float64 restatement of the SIFT extractor (tests/sift_ref.py) against truths it did not produce: analytic blobs, the
reference's own selection code (tests/golden/sift_select.npz), an exact 90 degree rotation, and the header.  No GPU."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sift_ref as R  # noqa: E402

from openglue_amd import _lib, build as og_build, synthetic as syn  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "sift_select.npz")
NAMES = ["og_sift_geometry", "og_sift_workspace_bytes", "og_sift_pyramid", "og_sift_detect", "og_sift_orient", "og_sift_describe",
         "og_sift_select", "og_sift_gather"]


@pytest.mark.parametrize("s", [2.0, 3.1, 4.5, 6.3])
def test_blob_position_and_scale(s):
    """A Gaussian blob of std s on a flat background: the DoG of a Gaussian blob peaks (in scale) where sigma^2 = (s^2 - 0.25) /
    2^(1/3) -- the 0.25 is the assumed input blur 0.5 squared, 2^(1/3) the ratio of adjacent scales.  The strongest keypoint within
    3 px of the centre must sit within 0.1 px of it (with the -0.25 correction of step 5; without it the error is 0.25 px) and
    within 5 % of that scale.  A float64 prototype measured <= 0.045 px and 0.995 .. 1.024: the bars are twice that."""
    H, W, cx, cy = 96, 128, 60.3, 47.6
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    img = 0.2 + 0.6 * np.exp(-((xx - cx) ** 2 + (yy - cy) ** 2) / (2 * s * s))
    _, dog = R.pyramid(R.quantize(img))
    _, kf = R.detect(dog)
    near = np.nonzero(np.hypot(kf[:, 0] - cx, kf[:, 1] - cy) < 3.0)[0]
    assert near.size, "no keypoint at the blob"
    k = kf[near[np.argmax(kf[near, 3])]]
    err = float(np.hypot(k[0] - cx, k[1] - cy))
    ratio = float(k[2] / 2.0 / np.sqrt((s * s - 0.25) / 2.0 ** (1.0 / 3.0)))
    print(f"blob s={s}: position error {err:.4f} px, scale ratio {ratio:.4f}")
    assert err <= 0.1
    assert 0.95 <= ratio <= 1.05


def _golden_cases():
    z = np.load(GOLDEN)
    for n in z["sizes"]:
        for di, d in enumerate(z["diameters"]):
            for mk in (-1, 512, int(n) + 10):
                for rs in (1, 0):
                    yield z, int(n), float(d), mk, bool(rs), f"n{n}_d{di}_k{mk}_r{rs}"


def test_selection_equals_the_reference():
    """select / lafs_from_keypoints / normalize_descriptors against the reference's detect_kpts_opencv, lafs_from_opencv_kpts and
    normalize_descriptors (base.py, run by tests/golden/make_golden_sift.py): kept sets equal, values to 1e-6 (relative to 1)."""
    cases = 0
    for z, n, d, mk, rs, name in _golden_cases():
        of, desc = R.synthetic_keypoints(n, seed=n)
        keep = R.select(of[:, :2], of[:, 4], np.arange(n), d, mk)
        assert np.array_equal(keep, z[name + "_keep"].astype(np.int64)), name
        ls, ds = int(z["row_stride"]), int(z["desc_stride"])
        np.testing.assert_allclose(R.lafs_from_keypoints(of[keep][::ls]), z[name + "_lafs"], rtol=1e-6, atol=1e-6, err_msg=name)
        np.testing.assert_allclose(R.normalize_descriptors(desc[keep][::ds], rs), z[name + "_desc"], rtol=1e-6, atol=1e-6, err_msg=name)
        cases += 1
    assert cases == 48


def test_greedy_chain():
    """every point suppresses the next: the greedy pass keeps every other one"""
    n = 50
    xy = np.stack([np.arange(n) * 3.0, np.zeros(n)], axis=1)
    keep = R.select(xy, np.linspace(1.0, 0.5, n), np.arange(n), 9.0, -1)
    assert np.array_equal(keep, np.arange(0, n, 2))


def test_rotation_by_90_degrees():
    """rot90 maps keypoints, angles (+90 degrees) and descriptors onto each other.  Checked on the first octave: the next octave takes
    every second pixel FROM 0, which a rotation turns into every second pixel from 1, so later octaves sample different pixels of the
    rotated image and are not images of each other.  Only keypoints with a response above 1e-6 are compared (extrema of rounding
    noise are not symmetric)."""
    H, W = 72, 96
    img = (syn.make_image(H, W, seed=5)[0, 0].numpy() * 255).round() / 255
    rot = np.rot90(img, -1)                      # new[i, j] = old[H - 1 - j, i]: (x, y) -> (H - 1 - y, x), directions turn by +90 degrees
    out = []
    for im in (img, rot):
        gauss, dog = R.pyramid(R.quantize(im))
        ki, kf = R.detect(dog)
        oi, of, _ = R.orient(gauss, ki, kf)
        m = (oi[:, 0] == 0) & (of[:, 4] > 1e-6)
        oi, of = oi[m], of[m]
        out.append((oi, of, R.describe(gauss, oi, of, quantize=False)))
    (oa, fa, da), (ob, fb, db) = out
    assert len(oa) == len(ob) and len(oa) >= 30
    mapped = np.stack([H - 1 - fa[:, 1].astype(np.float64), fa[:, 0].astype(np.float64)], axis=1)
    used = set()
    for i in range(len(oa)):
        ang = (float(fa[i, 3]) + 90.0) % 360.0
        dist = np.hypot(fb[:, 0] - mapped[i, 0], fb[:, 1] - mapped[i, 1])
        dang = np.abs((fb[:, 3].astype(np.float64) - ang + 180.0) % 360.0 - 180.0)
        j = np.nonzero((dist < 1e-4) & (dang < 1e-3) & (ob[:, 1] == oa[i, 1]))[0]
        assert j.size == 1, (i, fa[i], j)
        j = int(j[0])
        assert j not in used
        used.add(j)
        assert abs(float(fb[j, 2]) - float(fa[i, 2])) <= 1e-5 * float(fa[i, 2])
        assert abs(float(fb[j, 4]) - float(fa[i, 4])) <= 1e-6 * float(fa[i, 4]) + 1e-12
        assert np.abs(da[i] - db[j]).max() <= 1e-6, (i, np.abs(da[i] - db[j]).max())


def test_zero_descriptor_stays_zero():
    assert not np.isnan(R.finish_descriptor(np.zeros(128))).any()
    assert np.array_equal(R.normalize_descriptors(np.zeros((2, 128)), True), np.zeros((2, 128)))
    assert np.array_equal(R.normalize_descriptors(np.zeros((2, 128)), False), np.zeros((2, 128)))


def test_header_and_binding_hold_the_new_entries():
    header = open(os.path.join(ROOT, "include", "openglue_amd.h")).read()
    declared = set(re.findall(r"^\s*(?:int|size_t)\s+(og_\w+)\s*\(", header, flags=re.M))
    for name in NAMES:
        assert name in declared and name in _lib.SYMBOLS, name
    assert re.search(r"#define OG_ABI_VERSION 14\b", header) and _lib.OG_ABI_VERSION == 14      # additive: no bump
    assert "sift.hip" in og_build.SOURCES


def test_geometry_and_limits():
    lib = _lib.load()
    from openglue_amd import sift
    for H, W in ((64, 64), (97, 131), (120, 160), (480, 640)):
        g = sift.geometry(H, W)
        assert g.octaves == R.octave_sizes(H, W)
        assert g.cap == max(1024, H * W // 2) and g.cap2 == g.cap + g.cap // 4
        assert lib.og_sift_workspace_bytes(1, H, W) > 0
    assert len(sift.geometry(64, 64).octaves) == 4
    for B, H, W in ((1, 7, 64), (1, 64, 7), (1, 8193, 64), (0, 64, 64), (5, 1024, 1024)):
        assert lib.og_sift_workspace_bytes(B, H, W) == 0
    assert lib.og_sift_pyramid(1, 64, 64, None, None, None, None, None) == -1                     # OG_E_INVALID
    assert lib.og_sift_gather(1, 64, 64, -1, None, None, None, None, None, None, None) == -1


def test_argument_checks():
    import torch
    from openglue_amd.sift import SIFT
    with pytest.raises(RuntimeError):
        SIFT()(torch.zeros(1, 1, 64, 64))
    with pytest.raises(ValueError):
        SIFT()(torch.zeros(1, 3, 64, 64))
    with pytest.raises(ValueError):
        SIFT()(torch.zeros(1, 1, 4, 64))
    with pytest.raises(ValueError):
        SIFT(max_keypoints=2.5)(torch.zeros(1, 1, 64, 64))
    with pytest.raises(ValueError):
        SIFT(nms_diameter=float("nan"))(torch.zeros(1, 1, 64, 64))
