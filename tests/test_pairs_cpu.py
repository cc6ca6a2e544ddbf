"""CPU checks of the homography training pairs (openglue_amd.pairs, og_perspective_transform / og_warp_perspective_u8 /
og_homography_pairs): the numpy restatement in tests/pairs_ref.py against what it must mean geometrically, so that the GPU tests
compare against something known to be right; the refusals; the ABI; the compiled kernels' resources.  No kernel is launched here."""
import os
import re

import numpy as np
import pytest
import torch

from openglue_amd import _lib
from tests import pairs_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = {"og_perspective_transform", "og_warp_perspective_u8", "og_homography_pairs"}


def _frame(H, W, C, seed):
    return np.random.default_rng(seed).integers(0, 256, (1, H, W, C), dtype=np.uint8)


@pytest.mark.parametrize("C", [1, 3])
def test_identity_reproduces_the_frame(C):
    img = _frame(37, 53, C, 1)
    assert np.array_equal(ref.warp_perspective(img, np.eye(3)[None]), img)
    assert np.array_equal(ref.warp_perspective(img, np.eye(3)[None], (41, 29), (5, 3)), img[:, 3:32, 5:46])


@pytest.mark.parametrize("tx,ty", [(4, 0), (-3, 7), (0, -36), (60, 2)])
def test_integer_translation_shifts_and_pads_with_zeros(tx, ty):
    H, W = 37, 53
    img = _frame(H, W, 3, 2)
    M = np.array([[[1.0, 0.0, tx], [0.0, 1.0, ty], [0.0, 0.0, 1.0]]])
    exp = np.zeros_like(img)
    ys, xs = np.mgrid[0:H, 0:W]
    inside = (ys - ty >= 0) & (ys - ty < H) & (xs - tx >= 0) & (xs - tx < W)
    exp[0][inside] = img[0][(ys - ty)[inside], (xs - tx)[inside]]
    assert np.array_equal(ref.warp_perspective(img, M), exp)


def test_weights_sum_to_2_pow_15():
    fy, fx = np.mgrid[0:32, 0:32]
    w = ref.weights(fx, fy)
    assert all((v >= 0).all() for v in w) and (sum(w) == 32768).all()
    # ... and they are cv2's table: the product of the two 1-d linear weights, scaled to 15 bits, is already an integer
    assert np.array_equal(w[1], np.rint((fx / 32.0) * (1 - fy / 32.0) * 32768).astype(np.int64))


@pytest.mark.parametrize("solver", [ref.get_perspective_transform, ref.get_perspective_transform_eliminated])
def test_transform_maps_the_corners(solver):
    rng = np.random.default_rng(3)
    base = np.array([[0, 0], [0, 79], [95, 0], [95, 79]], np.float32)
    src = (base[None] + rng.integers(-12, 12, (50, 4, 2))).astype(np.float32)
    dst = (base[None] + rng.integers(-12, 12, (50, 4, 2))).astype(np.float32)
    M = solver(src, dst)
    p = np.concatenate([src.astype(np.float64), np.ones((50, 4, 1))], -1) @ M.transpose(0, 2, 1)
    err = np.abs(p[..., :2] / p[..., 2:] - dst).max()
    print(f"worst corner error {err:.3e} px")
    assert err <= 1e-9 and (M[:, 2, 2] == 1).all()


def test_both_solvers_agree_and_refuse_collinear_points():
    """np.linalg.solve and the stated elimination: the corners agree to 1e-7 px (measured about 1e-13), the matrices not to the bit;
    three collinear source points give M = 0 from both."""
    rng = np.random.default_rng(4)
    base = np.array([[0, 0], [0, 79], [95, 0], [95, 79]], np.float32)
    src = (base[None] + rng.integers(-12, 12, (50, 4, 2))).astype(np.float32)
    dst = np.broadcast_to(base, src.shape)
    A, B = ref.get_perspective_transform(src, dst), ref.get_perspective_transform_eliminated(src, dst)
    h = np.concatenate([src.astype(np.float64), np.ones((50, 4, 1))], -1)
    pa, pb = h @ A.transpose(0, 2, 1), h @ B.transpose(0, 2, 1)
    assert np.abs(pa[..., :2] / pa[..., 2:] - pb[..., :2] / pb[..., 2:]).max() <= 1e-7
    for bad in ([[0, 0], [1, 1], [2, 2], [0, 5]], [[0, 0], [10, 0], [25, 0], [7, 9]], [[3, 3], [3, 3], [9, 1], [2, 8]]):
        bad = np.array(bad, np.float32)
        assert not ref.get_perspective_transform(bad, base).any() and not ref.get_perspective_transform_eliminated(bad, base).any()


def test_zero_matrix_and_nan_are_defined():
    img = _frame(16, 20, 3, 5)
    out = ref.warp_perspective(img, np.zeros((1, 3, 3)))
    assert (out == img[0, 0, 0]).all()                                   # Mi = 0: every pixel samples (0, 0) with weight 32768
    out = ref.warp_perspective(img, np.full((1, 3, 3), np.nan))
    assert (out == 0).all()                                              # NaN coordinates go to INT_MIN: outside


def test_half_pixel_translation_hits_fraction_16():
    Mi = ref.invert3(np.array([[1, 0, 0.5], [0, 1, -0.5], [0, 0, 1.0]]))
    ys, xs = np.meshgrid(np.arange(9.0), np.arange(11.0), indexing="ij")
    X, Y = ref.source_xy(Mi, xs, ys)
    assert ((X & 31) == 16).all() and ((Y & 31) == 16).all()
    assert np.array_equal(X >> 5, xs.astype(np.int64) - 1) and np.array_equal(Y >> 5, ys.astype(np.int64))


def test_division_by_255_in_float32_equals_the_float64_one_rounded():
    """oxford_paris_dataset.py divides a FloatTensor by 255., megadepth_dataset.py a float64 array and rounds after: the same 256 floats"""
    v = np.arange(256)
    assert np.array_equal(ref.to_unit(v), (v / 255.0).astype(np.float32))


def _blob_frame(H, W, centres, sigma=1.5):
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float64)
    img = np.zeros((H, W))
    for cx, cy in centres:
        img += np.exp(-((xs - cx) ** 2 + (ys - cy) ** 2) / (2 * sigma * sigma))
    g = np.clip(np.rint(255 * img), 0, 255).astype(np.uint8)
    return np.repeat(g[None, :, :, None], 3, axis=3)


def test_h_true_relates_the_two_crops():
    """96 x 80 frame, offset 12, isolated Gaussian blobs (sigma 1.5): the intensity centroid of every blob in image1 lies within 0.5 px
    of H_true (p - offset), for the blobs that land at least 4 px inside the crop; 20 random offset draws.  (Bilinear sampling at 1/32 px
    and the byte quantisation of blob and warp account for what is seen: at most 0.36 px with these blobs and draws.)  A wrong corner
    order, a swapped direction or a missing crop origin gives many pixels."""
    H, W, o, R = 80, 96, 12, 7
    rng = np.random.default_rng(6)
    centres = [(x + rng.uniform(-2, 2), y + rng.uniform(-2, 2)) for y in range(11, 80, 19) for x in range(12, 96, 18)]
    frame = _blob_frame(H, W, centres)
    h, w = H - 2 * o, W - 2 * o
    worst, used = 0.0, 0
    for draw in range(20):
        wo = rng.integers(-o, o, (1, 4, 2)).astype(np.float32)
        for solver in (ref.get_perspective_transform, ref.get_perspective_transform_eliminated):
            image0, image1, H_true, _ = ref.homography_pairs(frame, o, wo, solver)
            assert image0.shape == image1.shape == (1, 1, h, w) and image0.dtype == image1.dtype == H_true.dtype == np.float32
            assert np.array_equal(image0[0, 0], (frame[0, o:H - o, o:W - o, 0] / 255.0).astype(np.float32))
            Ht = H_true[0].astype(np.float64)
            for cx, cy in centres:
                q = Ht @ np.array([cx - o, cy - o, 1.0])
                qx, qy = q[0] / q[2], q[1] / q[2]
                if not (4 <= qx <= w - 1 - 4 and 4 <= qy <= h - 1 - 4):
                    continue
                ix, iy = int(round(qx)), int(round(qy))
                x0, x1, y0, y1 = max(ix - R, 0), min(ix + R + 1, w), max(iy - R, 0), min(iy + R + 1, h)
                win = image1[0, 0, y0:y1, x0:x1].astype(np.float64)
                ys, xs = np.mgrid[y0:y1, x0:x1]
                assert win.sum() > 0
                mx, my = (win * xs).sum() / win.sum(), (win * ys).sum() / win.sum()
                worst = max(worst, float(np.hypot(mx - qx, my - qy)))
                used += 1
    print(f"worst centroid distance {worst:.3f} px over {used} blobs")
    assert used > 200 and worst <= 0.5


def test_warping_pairs_returns_the_warp_matrix():
    rng = np.random.default_rng(7)
    frames = rng.integers(0, 256, (2, 48, 64), dtype=np.uint8)
    wo = rng.integers(-10, 10, (2, 4, 2)).astype(np.float32)
    image0, image1, Hm, M = ref.warping_pairs(frames, wo)
    assert np.array_equal(image0[:, 0], (frames / 255.0).astype(np.float32)) and np.array_equal(Hm, M.astype(np.float32))
    assert np.array_equal(image1[:, 0], (ref.warp_perspective(frames[..., None], M)[..., 0] / 255.0).astype(np.float32))
    c = np.array([[0, 0], [0, 47], [63, 0], [63, 47]], np.float64)
    p = np.concatenate([c, np.ones((4, 1))], 1) @ M[0].T
    assert np.abs(p[:, :2] / p[:, 2:] - (c + wo[0])).max() <= 1e-9


def test_abi_version_and_symbol_sets():
    lib = _lib.load()
    assert _lib.OG_ABI_VERSION == 14 and lib.og_abi_version() == 14
    header = open(os.path.join(ROOT, "include", "openglue_amd.h")).read()
    assert re.search(r"#define OG_ABI_VERSION 14\b", header)
    declared = set(re.findall(r"^\s*(?:int|size_t)\s+(og_\w+)\s*\(", header, flags=re.M))
    assert NEW_SYMBOLS <= declared and NEW_SYMBOLS <= set(_lib.SYMBOLS)
    assert declared == set(_lib.SYMBOLS), declared ^ set(_lib.SYMBOLS)
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
    from openglue_amd import build as og_build
    assert "pairs.hip" in og_build.SOURCES
    assert "og_homography_pairs" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def test_entry_points_refuse_before_launching():
    """OG_E_INVALID (-1) for null pointers, OG_E_SHAPE (-2) for sizes and windows, OG_E_ALIGN (-3) for a misaligned matrix: all checked
    before anything is launched (the addresses are never dereferenced)."""
    lib = _lib.load()
    A = 0x10000
    assert lib.og_perspective_transform(1, None, A, A, None) == -1
    assert lib.og_perspective_transform(0, A, A, A, None) == -2
    assert lib.og_perspective_transform(1, A, A, A + 4, None) == -3
    warp = lambda **k: lib.og_warp_perspective_u8(k.get("B", 1), k.get("H", 8), k.get("W", 9), k.get("C", 3), k.get("src", A), k.get("M", A),
                                                  k.get("x0", 0), k.get("y0", 0), k.get("w", 9), k.get("h", 8), k.get("dst", A), None)
    for key in ("src", "M", "dst"):
        assert warp(**{key: None}) == -1, key
    for bad in (dict(C=2), dict(C=4), dict(B=0), dict(H=0), dict(w=0), dict(h=0), dict(x0=-1), dict(x0=1), dict(y0=1), dict(w=10), dict(W=40000)):
        assert warp(**bad) == -2, bad
    assert warp(M=A + 4) == -3
    pairs = lambda **k: lib.og_homography_pairs(k.get("B", 1), k.get("H", 8), k.get("W", 9), k.get("C", 3), k.get("frames", A), k.get("offset", 2),
                                                k.get("wo", A), k.get("i0", A), k.get("i1", A), k.get("Ht", A), k.get("ws", A), None)
    for key in ("frames", "i0", "i1", "Ht", "ws"):
        assert pairs(**{key: None}) == -1, key
    for bad in (dict(offset=-1), dict(offset=4), dict(C=2), dict(B=0)):
        assert pairs(**bad) == -2, bad
    assert pairs(ws=A + 4) == -3


def test_wrappers_refuse_before_any_device_is_touched():
    from openglue_amd import pairs
    u8 = lambda *s: torch.zeros(*s, dtype=torch.uint8)
    wo = torch.zeros(2, 4, 2)
    with pytest.raises(ValueError, match="uint8"):
        pairs.homography_pairs(torch.zeros(2, 16, 16, 3), 2, wo)
    with pytest.raises(ValueError, match=r"\[B, H, W\] or \[B, H, W, C\]"):
        pairs.homography_pairs(u8(16, 16), 2, wo)
    with pytest.raises(ValueError, match="C in"):
        pairs.homography_pairs(u8(2, 16, 16, 2), 2, wo)
    with pytest.raises(ValueError, match="non-negative"):
        pairs.homography_pairs(u8(2, 16, 16, 3), -1, wo)
    with pytest.raises(ValueError, match="non-negative"):
        pairs.homography_pairs(u8(2, 16, 16, 3), 2.0, wo)
    with pytest.raises(ValueError, match="below min"):
        pairs.homography_pairs(u8(2, 16, 20, 3), 8, wo)
    with pytest.raises(ValueError, match=r"warp_offset must be \[B, 4, 2\]"):
        pairs.homography_pairs(u8(2, 16, 16, 3), 2, torch.zeros(3, 4, 2))
    with pytest.raises(ValueError, match=r"warp_offset must be \[B, 4, 2\]"):
        pairs.warping_pairs(u8(2, 16, 16), 5, torch.zeros(2, 8))
    with pytest.raises(ValueError, match="C in"):
        pairs.warping_pairs(u8(2, 16, 16, 3), 5, wo)
    with pytest.raises(ValueError, match="non-negative"):
        pairs.warping_pairs(u8(2, 16, 16), -5, wo)
    with pytest.raises(ValueError, match=r"M must be \[B, 3, 3\]"):
        pairs.warp_perspective(u8(2, 16, 16), torch.zeros(3, 3))
    with pytest.raises(ValueError, match="uint8"):
        pairs.warp_perspective(torch.zeros(2, 16, 16), torch.zeros(2, 3, 3))
    for dsize, origin in (((17, 16), (0, 0)), ((16, 16), (1, 0)), ((4, 4), (0, 13)), ((0, 4), (0, 0)), ((4, 4), (-1, 0))):
        with pytest.raises(ValueError, match="inside the 16 x 16 frame"):
            pairs.warp_perspective(u8(2, 16, 16), torch.zeros(2, 3, 3), dsize, origin)
    with pytest.raises(ValueError, match=r"both be \[B, 4, 2\]"):
        pairs.get_perspective_transform(torch.zeros(2, 4, 2), torch.zeros(2, 4, 3))
    with pytest.raises(ValueError, match=r"both be \[B, 4, 2\]"):
        pairs.get_perspective_transform(torch.zeros(4, 2), torch.zeros(4, 2))
    # well-formed arguments that are not on the GPU: the library has no CPU path
    with pytest.raises(RuntimeError, match="GPU"):
        pairs.homography_pairs(u8(2, 16, 16, 3), 2, wo)
    with pytest.raises(RuntimeError, match="GPU"):
        pairs.get_perspective_transform(torch.zeros(2, 4, 2), torch.zeros(2, 4, 2))


def test_pairs_kernels_use_no_scratch(tmp_path):
    """Every kernel of pairs.hip compiles for gfx950 without scratch or spills (the figures DESIGN.md 4.13 quotes); the two image kernels keep
    eight waves per SIMD."""
    import subprocess
    from openglue_amd import build as og_build
    cmd = [og_build._hipcc(), *og_build.FLAGS, "-Rpass-analysis=kernel-resource-usage", "--cuda-device-only", "-c",
           os.path.join(og_build.CSRC, "pairs.hip"), "-o", str(tmp_path / "k.o")]
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=tmp_path)
    assert r.returncode == 0, r.stderr[-3000:]
    usage, name = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            usage[name] = {}
            continue
        m = re.search(r":\s{2,}([A-Za-z][^:]*): (\S+) \[-Rpass-analysis", line)
        if m and name:
            usage[name][m.group(1).strip()] = m.group(2)
    for kernel, instances, waves in (("perspective_transform_kernel", 1, 1), ("pairs_solve_kernel", 1, 1), ("warp_u8_kernel", 2, 8), ("pairs_kernel", 2, 8)):
        hits = [u for k, u in usage.items() if kernel in k]
        assert len(hits) == instances, (kernel, list(usage))
        for u in hits:
            print(f"{kernel}: SGPRs {u['TotalSGPRs']} VGPRs {u['VGPRs']} scratch {u['ScratchSize [bytes/lane]']} LDS {u['LDS Size [bytes/block]']} "
                  f"occupancy {u['Occupancy [waves/SIMD]']}")
            assert int(u["ScratchSize [bytes/lane]"]) == 0 and int(u["VGPRs Spill"]) == 0 and int(u["SGPRs Spill"]) == 0, (kernel, u)
            assert int(u["Occupancy [waves/SIMD]"]) >= waves, (kernel, u)
    assert len(usage) == 6, list(usage)
