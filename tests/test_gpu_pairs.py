"""GPU tests of the homography training pairs (openglue_amd.pairs, csrc/pairs.hip) against the numpy restatement tests/pairs_ref.py, which
tests/test_pairs_cpu.py checks on its own.  The warp and the pair items are compared bit for bit; the solver by the reprojection of the
corners against np.linalg.solve and bit for bit against the restated elimination.  Small shapes: the whole file takes seconds."""
import numpy as np
import pytest
import torch

from openglue_amd import features, pairs, supervision, synthetic as syn
from tests import pairs_ref as ref
from tests import supervision_ref

pytestmark = pytest.mark.gpu


def _gpu(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _reproject(M, pts):
    p = np.concatenate([pts.astype(np.float64), np.ones(pts.shape[:-1] + (1,))], -1) @ np.swapaxes(M, -1, -2)
    with np.errstate(all="ignore"):
        return p[..., :2] / p[..., 2:]


# ---------------------------------------------------------------- get_perspective_transform
def _quads():
    rng = np.random.default_rng(11)
    base = np.array([[0, 0], [0, 30], [40, 0], [40, 30]], np.float32)
    src = np.stack([base + rng.uniform(-6, 6, (4, 2)).astype(np.float32) for _ in range(5)])
    dst = np.stack([base + rng.uniform(-6, 6, (4, 2)).astype(np.float32) for _ in range(5)])
    dst[3] = src[3]                                          # the identity
    src[4] = base + rng.integers(-6, 6, (4, 2))              # whole pixels, so that the float32 sum below is exact
    dst[4] = src[4] + np.array([7.0, -3.0], np.float32)      # a pure translation
    return src, dst


def test_get_perspective_transform(gpu_device):
    src, dst = _quads()
    conds = [np.linalg.cond(ref.system(s, d)[0]) for s, d in zip(src, dst)]
    print("condition numbers", " ".join(f"{c:.2e}" for c in conds))
    assert max(conds) < 1e8                                   # before anything is launched
    want = ref.get_perspective_transform(src, dst)
    M = pairs.get_perspective_transform(_gpu(src, gpu_device), _gpu(dst, gpu_device))
    assert M.dtype == torch.float64 and M.shape == (5, 3, 3)
    got = M.cpu().numpy()
    err = np.abs(_reproject(got, src) - _reproject(want, src)).max()
    print(f"corner reprojection, kernel against np.linalg.solve: {err:.3e} px; against the destination: {np.abs(_reproject(got, src) - dst).max():.3e} px")
    assert err <= 1e-7
    assert (got[:, 2, 2] == 1).all()
    assert np.abs(got[3] - np.eye(3)).max() <= 1e-12 and np.abs(got[4] - np.array([[1, 0, 7], [0, 1, -3], [0, 0, 1.0]])).max() <= 1e-10
    assert np.array_equal(got, ref.get_perspective_transform_eliminated(src, dst))      # the stated order of operations, to the bit


def test_get_perspective_transform_degenerate(gpu_device):
    """three collinear source points: all zeros, finite; the well-posed system beside it in the batch is untouched"""
    src, dst = _quads()
    s = np.stack([np.array([[0, 0], [1, 1], [2, 2], [0, 5]], np.float32), src[0], np.array([[0, 0], [10, 0], [25, 0], [7, 9]], np.float32)])
    d = np.stack([dst[0], dst[0], dst[1]])
    got = pairs.get_perspective_transform(_gpu(s, gpu_device), _gpu(d, gpu_device)).cpu().numpy()
    assert np.isfinite(got).all() and not got[0].any() and not got[2].any()
    assert np.array_equal(got[1], ref.get_perspective_transform_eliminated(s[1], d[1]))
    assert not ref.get_perspective_transform(s, d)[[0, 2]].any()


# ---------------------------------------------------------------- warp_perspective
def _matrices(kind, B, H, W, rng):
    c = np.broadcast_to(np.array([[0, 0], [0, H - 1], [W - 1, 0], [W - 1, H - 1]], np.float32), (B, 4, 2))
    if kind == "mild":
        return ref.get_perspective_transform(c + rng.uniform(-5, 5, (B, 4, 2)).astype(np.float32), c)
    if kind == "strong":                                     # part of every window falls outside the source, on the negative side too
        return ref.get_perspective_transform(c + rng.uniform(8, 30, (B, 4, 2)).astype(np.float32) * rng.choice([-1.0, 1.0], (B, 1, 2)).astype(np.float32), c)
    if kind == "zero":
        return np.zeros((B, 3, 3))
    if kind == "half":                                       # X & 31 == 16 and Y & 31 == 16 on every pixel
        return np.broadcast_to(np.array([[1, 0, 0.5], [0, 1, -0.5], [0, 0, 1.0]]), (B, 3, 3)).copy()
    raise AssertionError(kind)


@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("H,W", [(37, 53), (64, 64)])
def test_warp_perspective_bit_identical(gpu_device, H, W, C):
    """matrices from the restatement's solver (np.linalg.solve), so that both sides see the same float64 M; B = 1 and B = 3 with a matrix
    per image; the full frame, an odd window, one row, one column"""
    rng = np.random.default_rng(100 * H + C)
    windows = [None, ((41, 29), (5, 3)), ((W, 1), (0, 7)), ((1, H), (9, 0))]
    saw_negative = saw_outside = False
    for B in (1, 3):
        img = rng.integers(0, 256, (B, H, W, C), dtype=np.uint8)
        frames = _gpu(img if C == 3 or B == 3 else img[..., 0], gpu_device)          # [B, H, W] is accepted for one channel
        for kind in ("mild", "strong", "zero", "half"):
            M = _matrices(kind, B, H, W, rng)
            Md = _gpu(M, gpu_device)
            for win in windows:
                dsize, origin = win or ((W, H), (0, 0))
                want = ref.warp_perspective(img, M, dsize, origin)
                got = pairs.warp_perspective(frames, Md, *(win or ()))
                assert got.dtype == torch.uint8
                got = got.cpu().numpy().reshape(want.shape)
                assert np.array_equal(got, want), (B, kind, win, int((got != want).sum()))
                if kind == "zero":
                    assert all((want[b] == img[b, 0, 0]).all() for b in range(B))
                if kind == "half":
                    xs, ys = np.meshgrid(np.arange(origin[0], origin[0] + dsize[0], dtype=np.float64), np.arange(origin[1], origin[1] + dsize[1], dtype=np.float64))
                    X, Y = ref.source_xy(ref.invert3(M[0]), xs, ys)
                    assert ((X & 31) == 16).all() and ((Y & 31) == 16).all()
                if kind == "strong" and win is None:
                    for b in range(B):
                        ys, xs = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
                        X, Y = ref.source_xy(ref.invert3(M[b]), xs, ys)
                        saw_negative |= bool((X < -32).any() or (Y < -32).any())
                        saw_outside |= bool(((X >> 5) >= W).any() or ((Y >> 5) >= H).any() or (X < -32).any() or (Y < -32).any())
    assert saw_negative and saw_outside


# ---------------------------------------------------------------- homography_pairs
B_, H_, W_, O_ = 3, 80, 96, 12


@pytest.fixture(scope="module")
def oxford():
    """frames, the given offsets (the extremes -offset and offset - 1 at every corner among them) and the restated item, computed once"""
    rng = np.random.default_rng(21)
    frames = rng.integers(0, 256, (B_, H_, W_, 3), dtype=np.uint8)
    frames[:, ::7] //= 3                                      # some structure besides noise
    wo = rng.integers(-O_, O_, (B_, 4, 2)).astype(np.float32)
    wo[0] = -O_
    wo[1] = O_ - 1
    wo[2, :, 0] = [-O_, O_ - 1, O_ - 1, -O_]
    wo[2, :, 1] = [O_ - 1, -O_, O_ - 1, -O_]
    image0, image1, H_true, H_warp = ref.homography_pairs(frames, O_, wo)
    return dict(frames=frames, wo=wo, image0=image0, image1=image1, H=H_true)


def _same(out, want):
    return (np.array_equal(out["image0"].cpu().numpy(), want["image0"]), np.array_equal(out["image1"].cpu().numpy(), want["image1"]),
            np.array_equal(out["transformation"]["H"].cpu().numpy(), want["H"]))


def test_homography_pairs_bit_identical(gpu_device, oxford):
    frames, wo = _gpu(oxford["frames"], gpu_device), _gpu(oxford["wo"], gpu_device)
    out = pairs.homography_pairs(frames, O_, wo)
    h, w = H_ - 2 * O_, W_ - 2 * O_
    assert out["image0"].shape == out["image1"].shape == (B_, 1, h, w) and out["image0"].dtype == out["image1"].dtype == torch.float32
    tr = out["transformation"]
    assert tr["type"] == ["perspective"] * B_ and tr["H"].shape == (B_, 3, 3) and tr["H"].dtype == torch.float32
    i1 = out["image1"].cpu().numpy()
    print("image1 values that differ from the restatement:", int((i1 != oxford["image1"]).sum()), "H entries:",
          int((tr["H"].cpu().numpy() != oxford["H"]).sum()))
    assert _same(out, oxford) == (True, True, True)
    # image0 is the grey of the plain crop
    crop = oxford["frames"][:, O_:H_ - O_, O_:W_ - O_].astype(np.int64)
    g = (9798 * crop[..., 0] + 19235 * crop[..., 1] + 3735 * crop[..., 2] + 16384) >> 15
    assert np.array_equal(out["image0"].cpu().numpy()[:, 0], g.astype(np.float32) / np.float32(255))
    # two calls give identical bytes
    again = pairs.homography_pairs(frames, O_, wo)
    for k in ("image0", "image1"):
        assert torch.equal(out[k], again[k])
    assert torch.equal(tr["H"], again["transformation"]["H"])
    # B calls of one frame give what one batched call gives
    for b in range(B_):
        one = pairs.homography_pairs(frames[b:b + 1], O_, wo[b:b + 1])
        assert torch.equal(one["image0"][0], out["image0"][b]) and torch.equal(one["image1"][0], out["image1"][b])
        assert torch.equal(one["transformation"]["H"][0], tr["H"][b])


def test_homography_pairs_grey_frames(gpu_device):
    """one channel, [B, H, W] and [B, H, W, 1], odd sizes, offset 0 and 5"""
    rng = np.random.default_rng(22)
    frames = rng.integers(0, 256, (2, 45, 67), dtype=np.uint8)
    for o in (0, 5):
        wo = rng.integers(-6, 6, (2, 4, 2)).astype(np.float32)
        image0, image1, H_true, _ = ref.homography_pairs(frames[..., None], o, wo)
        for f in (frames, frames[..., None]):
            out = pairs.homography_pairs(_gpu(f, gpu_device), o, _gpu(wo, gpu_device))
            assert _same(out, dict(image0=image0, image1=image1, H=H_true)) == (True, True, True)


def test_homography_pairs_random_offsets(gpu_device, oxford):
    frames = _gpu(oxford["frames"], gpu_device)
    gen = lambda seed: torch.Generator(device=gpu_device).manual_seed(seed)
    drawn = pairs._draw(B_, O_, gpu_device, gen(5))
    assert drawn.shape == (B_, 4, 2) and drawn.dtype == torch.float32
    assert torch.equal(drawn, drawn.round()) and float(drawn.min()) >= -O_ and float(drawn.max()) < O_       # np.random.randint's interval
    many = pairs._draw(400, 3, gpu_device, gen(6))
    assert sorted(many.unique().tolist()) == [-3.0, -2.0, -1.0, 0.0, 1.0, 2.0]
    a = pairs.homography_pairs(frames, O_, generator=gen(5))
    b = pairs.homography_pairs(frames, O_, generator=gen(5))
    c = pairs.homography_pairs(frames, O_, generator=gen(7))
    given = pairs.homography_pairs(frames, O_, drawn)
    for k in ("image0", "image1"):
        assert torch.equal(a[k], b[k]) and torch.equal(a[k], given[k])
    assert torch.equal(a["transformation"]["H"], b["transformation"]["H"]) and torch.equal(a["transformation"]["H"], given["transformation"]["H"])
    assert torch.equal(a["image0"], c["image0"])                                      # the crop does not depend on the draw
    assert not torch.equal(a["image1"], c["image1"]) and not torch.equal(a["transformation"]["H"], c["transformation"]["H"])


def test_warping_pairs_bit_identical(gpu_device):
    rng = np.random.default_rng(23)
    frames = rng.integers(0, 256, (2, 48, 64), dtype=np.uint8)
    wo = rng.integers(-10, 10, (2, 4, 2)).astype(np.float32)
    image0, image1, Hm, M = ref.warping_pairs(frames, wo)
    out = pairs.warping_pairs(_gpu(frames, gpu_device), 10, _gpu(wo, gpu_device))
    assert _same(out, dict(image0=image0, image1=image1, H=Hm)) == (True, True, True)
    assert out["transformation"]["type"] == ["perspective"] * 2
    # H is the warp matrix itself, in float32
    Md = pairs.get_perspective_transform(_gpu(ref.corners(48, 64, 0)[None].repeat(2, 0), gpu_device),
                                         _gpu(ref.corners(48, 64, 0)[None].repeat(2, 0) + wo, gpu_device))
    assert torch.equal(out["transformation"]["H"], Md.to(torch.float32))
    drawn = pairs.warping_pairs(_gpu(frames, gpu_device), 10, generator=torch.Generator(device=gpu_device).manual_seed(1))
    assert drawn["image1"].shape == (2, 1, 48, 64) and torch.equal(drawn["image0"], out["image0"])


# ---------------------------------------------------------------- frames -> pair -> extractor -> labels
def test_pairs_feed_the_extractor_and_the_labels(gpu_device):
    """one 240 x 320 frame, offset 24: the dictionary goes into generate_gt_matches exactly as returned, and the number of matched labels
    equals what tests/supervision_ref.py computes on the CPU from the same keypoints and the same H"""
    from openglue_amd.sift import SIFT
    H, W, o = 240, 320, 24
    rgb = torch.cat([syn.make_image(H, W, seed=51 + c) for c in range(3)], dim=1)             # [1, 3, H, W]
    frames = (rgb * 255).round().to(torch.uint8).permute(0, 2, 3, 1).contiguous().to(gpu_device)
    wo = torch.tensor([[[10, -7], [-12, 9], [-5, -20], [14, 6]]], dtype=torch.float32, device=gpu_device)
    data = pairs.homography_pairs(frames, o, wo)
    net = SIFT(max_keypoints=512)
    f = []
    for k in ("image0", "image1"):
        lafs, scores, desc = net(data[k])
        f.append(features.prepare_features_output(lafs, scores, desc, "none"))
    merged, y = supervision.generate_gt_matches(data, f[0], f[1], 3.0)
    M, N = f[0]["keypoints"].shape[1], f[1]["keypoints"].shape[1]
    assert merged is not None and merged["transformation"] is data["transformation"] and merged["image0"] is data["image0"]
    assert y["gt_matches0"].shape == (1, M) and y["gt_matches1"].shape == (1, N) and y["gt_matches0"].dtype == torch.int64
    tr = {"type": ["perspective"], "H": data["transformation"]["H"].cpu()}
    g0, g1 = supervision_ref.gt_matches(f[0]["keypoints"].cpu(), f[1]["keypoints"].cpu(), tr, 3.0)
    n0, n1 = int((y["gt_matches0"] >= 0).sum()), int((y["gt_matches1"] >= 0).sum())
    print(f"{M} / {N} keypoints, {n0} matched labels")
    assert n0 == int((g0 >= 0).sum()) and n1 == int((g1 >= 0).sum()) and n0 == n1
