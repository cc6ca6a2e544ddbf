"""GPU tests of the MegaDepth training pairs (openglue_amd.megadepth, csrc/megadepth.hip) against the numpy restatement
tests/megadepth_ref.py, which tests/test_megadepth_cpu.py checks on its own.  Everything is compared bit for bit.  Small shapes: the whole
file takes seconds."""
import numpy as np
import pytest
import torch

from openglue_amd import megadepth as md
from openglue_amd import supervision
from tests import megadepth_ref as ref
from tests import supervision_ref

pytestmark = pytest.mark.gpu

TARGET = (32, 24)
# (W, H): crop of the height, of the width, no crop (factor 2 down), crop of the width, up-scaling, the identity up to one column, odd width
# up-scaled, a factor above 6
SIZES = [(37, 53), (53, 37), (64, 48), (90, 41), (16, 12), (33, 24), (31, 24), (200, 150)]


def _gpu(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _windows(dw, dh):
    """the full destination, an odd window, the last column, the last row (the last two sit on the s >= src - 1 clamp)"""
    return [None, ((3, 2), (dw - 7, dh - 5)), ((dw - 1, 0), (1, dh)), ((0, dh - 1), (dw, 1))]


# ---------------------------------------------------------------- primitives
@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("W,H", SIZES)
def test_resize_linear_u8_bit_identical(gpu_device, W, H, C):
    dw, dh = md.crop_plan((W, H), TARGET)[:2]
    rng = np.random.default_rng(1000 * W + 10 * H + C)
    for B in (1, 3):
        img = rng.integers(0, 256, (B, H, W, C), dtype=np.uint8)
        frames = _gpu(img if C == 3 or B == 3 else img[..., 0], gpu_device)          # [B, H, W] is accepted for one channel
        for win in _windows(dw, dh):
            origin, window = win or ((0, 0), None)
            want = ref.resize_linear_u8(img, (dw, dh), origin, window)
            got = md.resize_linear_u8(frames, (dw, dh), origin, window)
            assert got.dtype == torch.uint8
            got = got.cpu().numpy().reshape(want.shape)
            assert np.array_equal(got, want), (B, win, int((got != want).sum()))


@pytest.mark.parametrize("interpolation", ["linear", "nearest"])
@pytest.mark.parametrize("W,H", SIZES)
def test_resize_f32_bit_identical(gpu_device, W, H, interpolation):
    dw, dh = md.crop_plan((W, H), TARGET)[:2]
    rng = np.random.default_rng(2000 * W + 10 * H)
    for B in (1, 3):
        maps = rng.uniform(0.0, 30.0, (B, H, W)).astype(np.float32)
        maps[:, ::5, ::3] = 0.0                                                       # holes, as MegaDepth's maps have
        d = _gpu(maps, gpu_device)
        for win in _windows(dw, dh):
            origin, window = win or ((0, 0), None)
            want = ref.resize_f32(maps, (dw, dh), interpolation, origin, window)
            got = md.resize_f32(d, (dw, dh), interpolation, origin, window)
            assert got.dtype == torch.float32 and got.shape == want.shape
            assert np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32)), (B, win)


# ---------------------------------------------------------------- megadepth_pairs
def _K(rng, W, H):
    return np.array([[rng.uniform(0.8, 1.6) * W, 0, W / 2 + rng.uniform(-2, 2)], [0, rng.uniform(0.8, 1.6) * W, H / 2 + rng.uniform(-2, 2)], [0, 0, 1]], np.float32)


@pytest.fixture(scope="module")
def ragged():
    """three pairs from SIZES (RGB and grey frames mixed; both crop axes and no crop), computed once"""
    rng = np.random.default_rng(31)
    sizes0, sizes1 = [(37, 53), (90, 41), (64, 48)], [(200, 150), (31, 24), (53, 37)]
    side = lambda sizes, grey: dict(
        frames=[rng.integers(0, 256, (H, W) if i == grey else (H, W, 3), dtype=np.uint8) for i, (W, H) in enumerate(sizes)],
        depth=[np.where(rng.uniform(size=(H, W)) < 0.1, 0.0, rng.uniform(1.0, 30.0, (H, W))).astype(np.float32) for W, H in sizes],
        K=np.stack([_K(rng, W, H) for W, H in sizes]), sizes=sizes)
    s0, s1 = side(sizes0, 1), side(sizes1, 0)
    R = np.stack([np.eye(3, dtype=np.float32)] * 3)
    T = rng.normal(size=(3, 3)).astype(np.float32)
    return s0, s1, R, T


def _want(s0, s1, starts, interpolation):
    plans = [[md.crop_plan(sz, TARGET, start=None if starts is None else starts[k][i]) for i, sz in enumerate(s["sizes"])] for k, s in enumerate((s0, s1))]
    return ref.megadepth_pairs(s0["frames"], s1["frames"], s0["depth"], s1["depth"], s0["K"], s1["K"], TARGET, plans[0], plans[1], interpolation)


def _call(dev, s0, s1, R, T, idx=None, **kw):
    pick = lambda v: [_gpu(v[i], dev) for i in (range(len(v)) if idx is None else idx)]
    sel = slice(None) if idx is None else list(idx)
    return md.megadepth_pairs(pick(s0["frames"]), pick(s1["frames"]), pick(s0["depth"]), pick(s1["depth"]), _gpu(s0["K"][sel], dev), _gpu(s1["K"][sel], dev),
                              _gpu(R[sel], dev), _gpu(T[sel], dev), TARGET, **kw)


def _bits(out):
    tr = out["transformation"]
    return [t.cpu().numpy() for t in (out["image0"], out["image1"], tr["depth0"], tr["depth1"], tr["K0"], tr["K1"])]


def _max_starts(s):
    return [(lambda p: (p[0] if p[2] == 0 else p[1]) - TARGET[p[2]])(md.crop_plan(sz, TARGET)) for sz in s["sizes"]]


def test_megadepth_pairs_bit_identical(gpu_device, ragged):
    s0, s1, R, T = ragged
    B = 3
    cases = [(None, "linear"), (None, "nearest"), (([0] * B, [0] * B), "linear"), ((_max_starts(s0), _max_starts(s1)), "linear")]
    assert max(_max_starts(s0)) > 0 and max(_max_starts(s1)) > 0
    for starts, interpolation in cases:
        want = _want(s0, s1, starts, interpolation)
        out = _call(gpu_device, s0, s1, R, T, starts=starts, depth_interpolation=interpolation)
        tr = out["transformation"]
        assert out["image0"].shape == out["image1"].shape == (B, 1, TARGET[1], TARGET[0]) and out["image0"].dtype == torch.float32
        assert tr["type"] == ["3d_reprojection"] * B and tr["depth0"].shape == tr["depth1"].shape == (B, TARGET[1], TARGET[0])
        assert tr["K0"].shape == tr["K1"].shape == tr["R"].shape == (B, 3, 3) and tr["T"].shape == (B, 3)
        assert all(t.dtype == torch.float32 and t.is_contiguous() for t in (tr["K0"], tr["K1"], tr["depth0"], tr["depth1"], tr["R"], tr["T"]))
        got = _bits(out)
        print(starts, interpolation, "values that differ from the restatement:", [int((g != w).sum()) for g, w in zip(got, want)])
        for g, w in zip(got, want):
            assert g.shape == w.shape and np.array_equal(g.view(np.uint32), w.view(np.uint32))
        assert np.array_equal(tr["R"].cpu().numpy(), R) and np.array_equal(tr["T"].cpu().numpy(), T)
    # two calls give identical bits; each pair alone equals its slice of the batch
    out = _call(gpu_device, s0, s1, R, T)
    again = _call(gpu_device, s0, s1, R, T)
    assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(_bits(out), _bits(again)))
    for b in range(B):
        one = _call(gpu_device, s0, s1, R, T, idx=[b])
        assert all(np.array_equal(a[0].view(np.uint32), w[b].view(np.uint32)) for a, w in zip(_bits(one), _bits(out)))


def test_megadepth_pairs_random_crop(gpu_device, ragged):
    s0, s1, R, T = ragged
    gen = lambda seed: torch.Generator().manual_seed(seed)
    a = _call(gpu_device, s0, s1, R, T, random_crop=True, generator=gen(3))
    b = _call(gpu_device, s0, s1, R, T, random_crop=True, generator=gen(3))
    assert all(np.array_equal(x, y) for x, y in zip(_bits(a), _bits(b)))
    g = gen(3)
    starts = [[md.crop_plan(sz, TARGET, random_crop=True, generator=g)[3] for sz in s["sizes"]] for s in (s0, s1)]
    given = _call(gpu_device, s0, s1, R, T, starts=starts)
    assert all(np.array_equal(x, y) for x, y in zip(_bits(a), _bits(given)))
    others = [_bits(_call(gpu_device, s0, s1, R, T, random_crop=True, generator=gen(seed)))[0] for seed in (4, 5, 6)]
    assert any(not np.array_equal(o, _bits(a)[0]) for o in others)


# ---------------------------------------------------------------- megadepth_feature_pairs
NUM_KPTS, DESC = 32, 16


def _image(rng, n, image_size, orig_size, ties=False, outside=False, start=0, axis=0):
    iw, ih = image_size
    lafs = rng.uniform(-1, 1, (n, 2, 3)).astype(np.float32)
    lafs[:, 0, 2] = rng.uniform(0, iw - 1e-3, n)
    lafs[:, 1, 2] = rng.uniform(0, ih - 1e-3, n)
    if outside and n:                                          # every keypoint left of / above the crop
        lafs[:, axis, 2] = rng.uniform(0, max(start - 1e-3, 0), n)
    scores = rng.uniform(0, 1, n).astype(np.float32)
    if ties:
        scores = (rng.integers(0, 6, n) / 8).astype(np.float32)            # six values over n keypoints: ties across the selection's edge
    desc = rng.normal(size=(n, DESC)).astype(np.float32)
    depth = np.where(rng.uniform(size=orig_size[::-1]) < 0.1, 0.0, rng.uniform(1, 30, orig_size[::-1])).astype(np.float32)
    return lafs, scores, desc, image_size, orig_size, depth, _K(rng, *orig_size)


@pytest.fixture(scope="module")
def cached():
    """B = 4: N of 0, 5, 40 and 70 on side 0 (empty, padded, selected by the width crop or not), ties and an all-outside image on side 1"""
    rng = np.random.default_rng(41)
    side0 = [_image(rng, 0, (52, 24), (97, 45)), _image(rng, 5, (32, 45), (61, 86)), _image(rng, 40, (32, 24), (64, 48)), _image(rng, 70, (52, 24), (104, 48))]
    side1 = [_image(rng, 70, (32, 45), (61, 86), ties=True), _image(rng, 40, (52, 24), (97, 45), outside=True, start=10),
             _image(rng, 70, (32, 24), (32, 24), ties=True), _image(rng, 40, (32, 45), (128, 180), ties=True)]
    R = np.stack([np.eye(3, dtype=np.float32)] * 4)
    T = rng.normal(size=(4, 3)).astype(np.float32)
    return side0, side1, R, T


def _dicts(items, dev, idx=None):
    return [dict(lafs=_gpu(it[0], dev), scores=_gpu(it[1], dev), descriptors=_gpu(it[2], dev), image_size=it[3], orig_size=it[4], depth=_gpu(it[5], dev),
                 K=_gpu(it[6], dev)) for i, it in enumerate(items) if idx is None or i in idx]


def _fbits(out):
    tr = out["transformation"]
    return [out[f"{k}{s}"].cpu().numpy() for s in (0, 1) for k in ("lafs", "scores", "descriptors")] + \
           [tr[k].cpu().numpy() for k in ("depth0", "depth1", "K0", "K1")]


def _fwant(side0, side1, starts, keys=None):
    w = []
    for s, items in enumerate((side0, side1)):
        plans = [md.feature_crop_plan(it[3], TARGET, start=None if starts is None else starts[s][i]) for i, it in enumerate(items)]
        w.append(ref.feature_pairs_side(items, TARGET, NUM_KPTS, plans, None if keys is None else keys[s]))
    (l0, s0, d0, p0, k0), (l1, s1, d1, p1, k1) = w
    return [l0, s0, d0, l1, s1, d1, p0, p1, k0, k1]


def test_megadepth_feature_pairs_bit_identical(gpu_device, cached):
    side0, side1, R, T = cached
    B = 4
    max_starts = [[max(it[3][0] - TARGET[0], 0) or max(it[3][1] - TARGET[1], 0) for it in items] for items in (side0, side1)]
    for starts in (None, ([0] * B, [0] * B), max_starts):
        want = _fwant(side0, side1, starts)
        out = md.megadepth_feature_pairs(_dicts(side0, gpu_device), _dicts(side1, gpu_device), _gpu(R, gpu_device), _gpu(T, gpu_device), TARGET, NUM_KPTS,
                                         starts=starts)
        assert out["lafs0"].shape == (B, NUM_KPTS, 2, 3) and out["descriptors1"].shape == (B, NUM_KPTS, DESC) and out["scores0"].shape == (B, NUM_KPTS)
        assert out["image0_size"] == TARGET and out["image1_size"] == TARGET and out["transformation"]["type"] == ["3d_reprojection"]
        assert out["transformation"]["depth0"].shape == (B, NUM_KPTS)
        got = _fbits(out)
        print(starts, "values that differ from the restatement:", [int((g != w).sum()) for g, w in zip(got, want)])
        for g, w in zip(got, want):
            assert g.shape == w.shape and np.array_equal(g.view(np.uint32), w.view(np.uint32))
    want = _fwant(side0, side1, None)
    # what the fixture is there for: an empty image, a padded one, selected ones, ties across the edge of the selection, all outside
    assert not want[1][0].any() and 0 < np.count_nonzero(want[1][1]) <= 5 and np.count_nonzero(want[1][3]) == NUM_KPTS
    assert not want[4][1].any() and not want[7][1].any()
    s, (axis, start) = want[4][0], md.feature_crop_plan(side1[0][3], TARGET)
    y = side1[0][0][:, axis, 2]
    left = side1[0][1][(y >= start) & (y < start + TARGET[axis])]
    assert (s[:-1] >= s[1:]).all() and (s[:-1] == s[1:]).any() and np.count_nonzero(left == s[-1]) > np.count_nonzero(s == s[-1])
    # generate_gt_matches takes the per-keypoint depth as it is
    assert out["transformation"]["depth1"].dtype == torch.float32 and out["transformation"]["depth1"].is_contiguous()
    # each pair alone equals its slice of the batch
    full = _fbits(md.megadepth_feature_pairs(_dicts(side0, gpu_device), _dicts(side1, gpu_device), _gpu(R, gpu_device), _gpu(T, gpu_device), TARGET, NUM_KPTS))
    for b in range(B):
        one = _fbits(md.megadepth_feature_pairs(_dicts(side0, gpu_device, [b]), _dicts(side1, gpu_device, [b]), _gpu(R[b:b + 1], gpu_device),
                                                _gpu(T[b:b + 1], gpu_device), TARGET, NUM_KPTS))
        assert all(np.array_equal(a[0].view(np.uint32), w[b].view(np.uint32)) for a, w in zip(one, full))


def test_megadepth_feature_pairs_given_and_random_keys(gpu_device, cached):
    side0, side1, R, T = cached
    rng = np.random.default_rng(43)
    keys = [[rng.integers(0, 9, len(it[1])).astype(np.float32) for it in items] for items in (side0, side1)]
    args = lambda: (_dicts(side0, gpu_device), _dicts(side1, gpu_device), _gpu(R, gpu_device), _gpu(T, gpu_device), TARGET, NUM_KPTS)
    out = md.megadepth_feature_pairs(*args(), keys=tuple([_gpu(k, gpu_device) for k in ks] for ks in keys))
    for g, w in zip(_fbits(out), _fwant(side0, side1, None, keys)):
        assert np.array_equal(g.view(np.uint32), w.view(np.uint32))
    gen = lambda seed: torch.Generator(device=gpu_device).manual_seed(seed)
    a = md.megadepth_feature_pairs(*args(), random=True, generator=gen(1))
    b = md.megadepth_feature_pairs(*args(), random=True, generator=gen(1))
    c = md.megadepth_feature_pairs(*args(), random=True, generator=gen(2))
    assert all(np.array_equal(x, y) for x, y in zip(_fbits(a), _fbits(b)))
    # side 0, image 3: 70 keypoints of which more than 32 survive the crop; the kept ones are 32 distinct survivors
    lafs, scores, desc = side0[3][:3]
    axis, start = md.feature_crop_plan((52, 24), TARGET)
    inside = (lafs[:, 0, 2] >= start) & (lafs[:, 0, 2] < start + TARGET[0])
    assert axis == 0 and inside.sum() > NUM_KPTS
    survivors = {d.tobytes() for d in desc[inside]}
    kept = [{d.tobytes() for d in o["descriptors0"][3].cpu().numpy()} for o in (a, c)]
    assert all(len(k) == NUM_KPTS and k <= survivors for k in kept) and kept[0] != kept[1]
    # at most num_keypoints survivors: nothing is drawn away, the order stays
    assert np.array_equal(a["scores0"][1].cpu().numpy(), _fwant(side0, side1, None)[1][1])


# ---------------------------------------------------------------- frames -> item -> labels
def test_pairs_feed_the_labels(gpu_device):
    """frames1 = frames0, R = I, T = 0, constant depth: every keypoint at a whole pixel reprojects onto itself, so generate_gt_matches fed with
    the item as returned labels keypoint i as matched to i -- and tests/supervision_ref.py says the same of the restatement's item"""
    rng = np.random.default_rng(51)
    sizes = [(90, 41), (37, 53)]
    frames = [rng.integers(0, 256, (H, W, 3), dtype=np.uint8) for W, H in sizes]
    depth = [np.full((H, W), 4.0, np.float32) for W, H in sizes]
    K = np.stack([_K(rng, W, H) for W, H in sizes])
    R, T = np.stack([np.eye(3, dtype=np.float32)] * 2), np.zeros((2, 3), np.float32)
    g = lambda v: [_gpu(a, gpu_device) for a in v]
    data = md.megadepth_pairs(g(frames), g(frames), g(depth), g(depth), _gpu(K, gpu_device), _gpu(K, gpu_device), _gpu(R, gpu_device), _gpu(T, gpu_device), TARGET)
    idx = np.stack([rng.choice(TARGET[0] * TARGET[1], 30, replace=False) for _ in sizes])
    kp = np.stack([idx % TARGET[0], idx // TARGET[0]], -1).astype(np.float32)          # distinct whole pixels, [2, 30, 2]
    n = kp.shape[1]
    feats = lambda: {"keypoints": _gpu(kp, gpu_device), "local_descriptors": torch.zeros(2, n, 8, device=gpu_device), "side_info": torch.zeros(2, n, 1, device=gpu_device)}
    merged, y = supervision.generate_gt_matches(data, feats(), feats(), 3.0)
    assert merged["transformation"] is data["transformation"] and merged["image0"] is data["image0"]
    want = np.broadcast_to(np.arange(n), (2, n))
    assert np.array_equal(y["gt_matches0"].cpu().numpy(), want) and np.array_equal(y["gt_matches1"].cpu().numpy(), want)
    plans = [md.crop_plan(sz, TARGET) for sz in sizes]
    i0, i1, d0, d1, k0, k1 = ref.megadepth_pairs(frames, frames, depth, depth, K, K, TARGET, plans, plans)
    tr = {"type": ["3d_reprojection"] * 2, "K0": torch.from_numpy(k0), "K1": torch.from_numpy(k1), "R": torch.from_numpy(R), "T": torch.from_numpy(T),
          "depth0": torch.from_numpy(d0), "depth1": torch.from_numpy(d1)}
    g0, g1 = supervision_ref.gt_matches(torch.from_numpy(kp), torch.from_numpy(kp), tr, 3.0)
    assert np.array_equal(g0.numpy(), want) and np.array_equal(g1.numpy(), want)
