"""CPU checks of the MegaDepth training pairs (openglue_amd.megadepth, og_resize_linear_u8 / og_resize_f32 / og_megadepth_pairs /
og_megadepth_features): the numpy restatement in tests/megadepth_ref.py against what it must mean, so that the GPU tests compare against
something known to be right; the host-side plans against a literal transcription of the reference's branches; the refusals; the ABI; the
compiled kernels' resources.  No kernel is launched here."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from openglue_amd import _lib
from openglue_amd import megadepth as md
from tests import megadepth_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = {"og_resize_linear_u8", "og_resize_f32", "og_megadepth_pairs", "og_megadepth_features"}
# (W, H) -> (dw, dh): up-scaling, down-scaling by more than 2, the identity, odd sizes, one axis up and the other down
SHAPES = [((37, 53), (32, 45)), ((53, 37), (34, 24)), ((64, 48), (32, 24)), ((90, 41), (52, 24)), ((16, 12), (32, 24)), ((33, 24), (33, 24)),
          ((200, 150), (32, 24)), ((31, 24), (40, 17))]


def _bilinear64(a, dsize):
    """float64 F.interpolate(bilinear, align_corners=False) of [B, H, W(, C)] to dsize = (dw, dh)"""
    t = torch.from_numpy(np.asarray(a, np.float64))
    t = t[:, None] if t.dim() == 3 else t.permute(0, 3, 1, 2)
    out = F.interpolate(t, size=(dsize[1], dsize[0]), mode="bilinear", align_corners=False)
    return (out[:, 0] if a.ndim == 3 else out.permute(0, 2, 3, 1)).numpy()


@pytest.mark.parametrize("C", [1, 3])
def test_resize_linear_u8_is_bilinear_within_one_level(C):
    """11-bit coefficients (each off by at most 2^-12), the >> 4, >> 16 and >> 2 truncations and the final rounding keep the result within
    one grey level of the exact bilinear value; 0.76 seen on these shapes"""
    rng = np.random.default_rng(1)
    worst = 0.0
    for (W, H), dsize in SHAPES:
        img = rng.integers(0, 256, (2, H, W) if C == 1 else (2, H, W, C), dtype=np.uint8)
        got = ref.resize_linear_u8(img, dsize)
        assert got.dtype == np.uint8 and got.shape[1:3] == dsize[::-1]
        worst = max(worst, float(np.abs(got.astype(np.float64) - _bilinear64(img, dsize)).max()))
    print(f"largest difference from float64 bilinear: {worst:.3f} grey levels")
    assert worst <= 1.0


def test_resize_linear_u8_identity_constant_and_window():
    rng = np.random.default_rng(2)
    img = rng.integers(0, 256, (2, 24, 33, 3), dtype=np.uint8)
    assert np.array_equal(ref.resize_linear_u8(img, (33, 24)), img)
    for v in (0, 1, 127, 255):
        for (W, H), dsize in SHAPES:
            assert (ref.resize_linear_u8(np.full((1, H, W), v, np.uint8), dsize) == v).all(), (v, W, H)
    full = ref.resize_linear_u8(img, (52, 31))
    assert np.array_equal(ref.resize_linear_u8(img, (52, 31), (5, 3), (41, 17)), full[:, 3:20, 5:46])
    assert np.array_equal(ref.resize_linear_u8(img, (52, 31), (51, 30)), full[:, 30:, 51:])


def test_taps_clamp_at_both_ends():
    for src, dst in ((12, 24), (16, 32), (150, 24), (24, 24), (1, 5), (5, 1)):
        s0, s1, f = ref.linear_taps(src, dst)
        assert s0.min() >= 0 and s1.max() <= src - 1 and ((s1 == s0) | (s1 == s0 + 1)).all()
        assert f.dtype == np.float32 and (f >= 0).all() and (f < 1).all() and (f[s0 == src - 1] == 0).all()
    s0, s1, f = ref.linear_taps(12, 24)                     # up-scaling by 2: d = 0 lies at -0.25 (clamped), d = 23 at 11.25 (clamped)
    assert s0[0] == 0 and f[0] == 0 and s0[-1] == 11 and f[-1] == 0 and f[1] == np.float32(0.25)


def test_resize_f32_linear_is_bilinear():
    """float32 coordinates carry an error of at most 2^-24 * max(W, H) <= 2^-16 pixel per axis, which moves the value by at most that times
    the largest step between neighbours; the four products and two sums add a few ulp of the largest value"""
    rng = np.random.default_rng(3)
    worst = 0.0
    for (W, H), dsize in SHAPES:
        m = rng.uniform(0.5, 20.0, (2, H, W)).astype(np.float32)
        got = ref.resize_f32(m, dsize, "linear")
        assert got.dtype == np.float32
        err = float(np.abs(got.astype(np.float64) - _bilinear64(m, dsize)).max())
        bound = 2 * 2.0 ** -16 * 19.5 + 8 * 2.0 ** -24 * 20.0
        worst = max(worst, err / bound)
        assert err <= bound, (W, H, dsize, err)
    print(f"largest error / bound: {worst:.3f}")
    m = rng.uniform(0.5, 20.0, (1, 24, 33)).astype(np.float32)
    assert np.array_equal(ref.resize_f32(m, (33, 24), "linear"), m)


def test_resize_f32_nearest_equals_the_loop():
    rng = np.random.default_rng(4)
    for (W, H), (dw, dh) in SHAPES:
        m = rng.uniform(0.0, 20.0, (1, H, W)).astype(np.float32)
        want = np.empty((dh, dw), np.float32)
        for y in range(dh):
            for x in range(dw):
                sy = min(int(np.floor(y * (1.0 / (dh / H)))), H - 1)
                sx = min(int(np.floor(x * (1.0 / (dw / W)))), W - 1)
                want[y, x] = m[0, sy, sx]
        assert np.array_equal(ref.resize_f32(m, (dw, dh), "nearest")[0], want)
        assert np.array_equal(ref.resize_f32(m, (dw, dh), "nearest", (1, 2), (dw - 1, dh - 2))[0], want[2:, 1:])


# ---------------------------------------------------------------- the plans
def _reference_plan(size, target_size, random_crop, randint):
    """data/megadepth_dataset.py:134-176, the branches as they stand there; randint stands for np.random.randint"""
    current_ratio = size[0] / size[1]
    target_ratio = target_size[0] / target_size[1]
    if current_ratio > target_ratio:
        resize_height = target_size[1]
        resize_width = int(current_ratio * resize_height)
        if random_crop:
            start_width = randint(0, max(resize_width - target_size[0], 1))
        else:
            start_width = (resize_width - target_size[0]) // 2
        return resize_width, resize_height, 0, start_width
    else:
        resize_width = target_size[0]
        resize_height = int(resize_width / current_ratio)
        if random_crop:
            start_height = randint(0, max(resize_height - target_size[1], 1))
        else:
            start_height = (resize_height - target_size[1]) // 2
        return resize_width, resize_height, 1, start_height


def test_crop_plan_follows_the_reference():
    target = (32, 24)
    sizes = [(37, 53), (53, 37), (64, 48), (90, 41), (16, 12), (33, 24), (31, 24), (200, 150), (1600, 1200), (1600, 1067), (1067, 1600), (32, 24)]
    axes = set()
    for size in sizes:
        want = _reference_plan(size, target, False, None)
        assert md.crop_plan(size, target) == want, size
        axes.add((want[2], np.sign(size[0] / size[1] - target[0] / target[1])))
    assert axes == {(0, 1.0), (1, -1.0), (1, 0.0)}                     # ratio above, below and equal to the target's
    for size, tgt in (((1600, 1200), (960, 720)), ((1600, 1067), (960, 720)), ((1200, 1600), (960, 720))):
        assert md.crop_plan(size, tgt) == _reference_plan(size, tgt, False, None)
    # the random start covers [0, max(resized - target, 1)) and nothing else; with no room it is 0
    rw, rh, axis, _ = md.crop_plan((90, 41), target)
    assert (rw, rh, axis) == (52, 24, 0)
    g = torch.Generator().manual_seed(5)
    seen = {md.crop_plan((90, 41), target, random_crop=True, generator=g)[3] for _ in range(600)}
    assert seen == set(range(0, 20))
    assert md.crop_plan((90, 41), target, random_crop=True, generator=torch.Generator().manual_seed(9)) == \
        md.crop_plan((90, 41), target, random_crop=True, generator=torch.Generator().manual_seed(9))
    for size in ((64, 48), (33, 24)):                                  # resized == target on the cropped axis: max(0, 1) = 1, start 0
        plan = md.crop_plan(size, target, random_crop=True, generator=g)
        assert plan == _reference_plan(size, target, True, lambda lo, hi: 0) and plan[3] == 0
    assert md.crop_plan((90, 41), target, start=0)[3] == 0 and md.crop_plan((90, 41), target, start=20)[3] == 20
    for bad in (-1, 21, 1.5):
        with pytest.raises(ValueError, match="start"):
            md.crop_plan((90, 41), target, start=bad)
    with pytest.raises(ValueError, match="positive"):
        md.crop_plan((0, 41), target)
    with pytest.raises(ValueError, match="two integers"):
        md.crop_plan((90,), target)


def test_crop_plan_never_falls_below_the_target(monkeypatch):
    """a coarse sweep of the sizes 20..2000 at three targets: no resized side falls below the target; the check that would catch one is
    exercised with an int() that truncates one too far"""
    for target in ((960, 720), (32, 24), (40, 24)):
        for w in range(20, 2001, 61):
            for h in range(20, 2001, 67):
                rw, rh, axis, start = md.crop_plan((w, h), target)
                assert rw >= target[0] and rh >= target[1] and start >= 0
    monkeypatch.setattr(md, "int", lambda v: int(v) - 1 if isinstance(v, float) else int(v), raising=False)
    with pytest.raises(ValueError, match="falls below the target"):
        md.crop_plan((64, 48), (32, 24))
    with pytest.raises(ValueError, match="falls below the target"):
        md.crop_plan((66, 24), (33, 12))


def test_feature_crop_plan_follows_the_reference():
    t = (32, 24)
    assert md.feature_crop_plan((52, 24), t) == (0, 10)
    assert md.feature_crop_plan((52, 40), t) == (0, 10)                 # the width is tried first
    assert md.feature_crop_plan((32, 45), t) == (1, 10)
    assert md.feature_crop_plan((32, 24), t) == (-1, 0) and md.feature_crop_plan((30, 20), t) == (-1, 0)
    g = torch.Generator().manual_seed(6)
    assert {md.feature_crop_plan((52, 24), t, random_crop=True, generator=g)[1] for _ in range(600)} == set(range(0, 20))   # [0, image - target)
    assert {md.feature_crop_plan((32, 27), t, random_crop=True, generator=g) for _ in range(100)} == {(1, 0), (1, 1), (1, 2)}
    assert md.feature_crop_plan((52, 24), t, start=20) == (0, 20)
    with pytest.raises(ValueError, match="start"):
        md.feature_crop_plan((52, 24), t, start=21)
    with pytest.raises(ValueError, match="nothing to crop"):
        md.feature_crop_plan((32, 24), t, start=1)


def test_K_is_the_float32_product():
    rng = np.random.default_rng(7)
    for size, resized, axis, start in (((1600, 1067), (1079, 720), 0, 59), ((37, 53), (32, 45), 1, 10), ((64, 48), (32, 24), 1, 0), ((33, 24), (33, 24), -1, 0)):
        K = np.array([[rng.uniform(500, 2000), 0, size[0] / 2 + rng.uniform(-5, 5)], [0, rng.uniform(500, 2000), size[1] / 2], [0, 0, 1]], np.float32)
        got = ref.scale_K(K, size, resized, axis, start)
        S = np.diag([resized[0] / size[0], resized[1] / size[1], 1.0]).astype(np.float32)
        want = np.zeros((3, 3), np.float32)
        for r in range(3):
            for c in range(3):
                acc = np.float32(0)
                for k in range(3):
                    acc = np.float32(acc + np.float32(S[r, k] * K[k, c]))
                want[r, c] = acc
        if axis >= 0:
            want[axis, 2] = np.float32(want[axis, 2] - np.float32(start))
        assert got.dtype == np.float32 and np.array_equal(got, want)
        # ... and it still maps the same ray: a pixel p of the original lies at S p - shift in the crop
        p = np.array([size[0] * 0.3, size[1] * 0.6, 1.0])
        ray = np.linalg.inv(K.astype(np.float64)) @ p
        q = got.astype(np.float64) @ ray
        shift = np.array([start if axis == 0 else 0, start if axis == 1 else 0])
        assert np.abs(q[:2] / q[2] - (p[:2] * np.array([resized[0] / size[0], resized[1] / size[1]]) - shift)).max() < 1e-2


# ---------------------------------------------------------------- the items
def test_online_item_is_grey_resize_crop():
    rng = np.random.default_rng(8)
    frame = rng.integers(0, 256, (41, 90, 3), dtype=np.uint8)
    depth = rng.uniform(1, 9, (41, 90)).astype(np.float32)
    K = np.array([[80, 0, 45], [0, 80, 20.5], [0, 0, 1]], np.float32)
    plan = md.crop_plan((90, 41), (32, 24), start=7)
    image, d, Kc = ref.megadepth_item(frame, depth, K, (32, 24), plan)
    v = frame.astype(np.int64)
    g = ((9798 * v[..., 0] + 19235 * v[..., 1] + 3735 * v[..., 2] + 16384) >> 15).astype(np.uint8)
    assert np.array_equal(image, ref.resize_linear_u8(g[None], (52, 24), (7, 0), (32, 24))[0].astype(np.float32) / np.float32(255))
    assert np.array_equal(d, ref.resize_f32(depth[None], (52, 24), "linear", (7, 0), (32, 24))[0])
    assert image.dtype == d.dtype == Kc.dtype == np.float32 and image.min() >= 0 and image.max() <= 1
    assert Kc[0, 2] == np.float32(np.float32(np.float32(52 / 90) * np.float32(45)) - np.float32(7))
    dn = ref.megadepth_item(frame, depth, K, (32, 24), plan, "nearest")[1]
    assert np.isin(dn, depth).all() and not np.isin(d, depth).all()


def _cached_image(rng, n, image_size, orig_size, D=8, distinct=True):
    iw, ih = image_size
    lafs = rng.uniform(-1, 1, (n, 2, 3)).astype(np.float32)
    lafs[:, 0, 2] = rng.uniform(0, iw - 1e-3, n)
    lafs[:, 1, 2] = rng.uniform(0, ih - 1e-3, n)
    scores = rng.permutation(n).astype(np.float32) / max(n, 1) if distinct else rng.integers(0, 4, n).astype(np.float32)
    desc = rng.normal(size=(n, D)).astype(np.float32)
    depth = rng.uniform(1, 9, (orig_size[1], orig_size[0])).astype(np.float32)
    K = np.array([[700, 0, orig_size[0] / 2], [0, 700, orig_size[1] / 2], [0, 0, 1]], np.float32)
    return lafs, scores, desc, image_size, orig_size, depth, K


def _reference_cached(item, target_size, k, start):
    """data/megadepth_dataset.py:223-258 and data/megadepth_datamodule.py:139-164 for one image, in torch as written there (distinct scores, so
    that torch.topk has one answer); the depth resize by an explicit nearest-neighbour loop"""
    lafs, scores, descriptors, image_size, orig_size, depth, K = item
    lafs = lafs.copy()
    dh, dw = depth.shape
    resized = np.empty((image_size[1], image_size[0]), np.float32)
    for y in range(image_size[1]):
        for x in range(image_size[0]):
            resized[y, x] = depth[min(int(np.floor(y * (1.0 / (image_size[1] / dh)))), dh - 1), min(int(np.floor(x * (1.0 / (image_size[0] / dw)))), dw - 1)]
    depth = resized
    scales = np.diag([image_size[0] / orig_size[0], image_size[1] / orig_size[1], 1.0]).astype(np.float32)
    K = np.dot(scales, K)
    if target_size[0] < image_size[0]:
        start_width = start
        end_width = start_width + target_size[0]
        depth = depth[:, start_width:end_width]
        kpts_crop_mask = (lafs[:, 0, 2] >= start_width) & (lafs[:, 0, 2] < end_width)
        K[0, 2] -= start_width
        lafs = lafs[kpts_crop_mask]
        lafs[:, 0, 2] -= start_width
        scores = scores[kpts_crop_mask]
        descriptors = descriptors[kpts_crop_mask]
    elif target_size[1] < image_size[1]:
        start_height = start
        end_height = start_height + target_size[1]
        depth = depth[start_height:end_height, :]
        kpts_crop_mask = (lafs[:, 1, 2] >= start_height) & (lafs[:, 1, 2] < end_height)
        K[1, 2] -= start_height
        lafs = lafs[kpts_crop_mask]
        lafs[:, 1, 2] -= start_height
        scores = scores[kpts_crop_mask]
        descriptors = descriptors[kpts_crop_mask]
    lafs, scores, descriptors, depth = (torch.from_numpy(np.ascontiguousarray(a)) for a in (lafs, scores, descriptors, depth))
    out = dict(lafs=torch.zeros(k, 2, 3), scores=torch.zeros(k), descriptors=torch.zeros(k, descriptors.size(1)), depth=torch.zeros(k))
    num_kpts = lafs.size(0)
    if num_kpts > k:
        idx = torch.topk(scores, k, dim=0).indices
        out["lafs"][:], out["scores"][:], out["descriptors"][:] = lafs[idx], scores[idx], descriptors[idx]
        out["depth"][:] = depth[out["lafs"][:, 1, 2].type(torch.int64), out["lafs"][:, 0, 2].type(torch.int64)]
    else:
        out["lafs"][:num_kpts], out["scores"][:num_kpts], out["descriptors"][:num_kpts] = lafs, scores, descriptors
        out["depth"][:num_kpts] = depth[lafs[:, 1, 2].type(torch.int64), lafs[:, 0, 2].type(torch.int64)]
    return {k_: v.numpy() for k_, v in out.items()}, K


@pytest.mark.parametrize("image_size,n", [((52, 24), 70), ((52, 24), 20), ((32, 45), 70), ((32, 45), 5), ((32, 24), 40), ((32, 24), 0)])
def test_cached_item_follows_the_reference(image_size, n):
    """more and fewer survivors than num_keypoints = 32, both crop axes and no crop"""
    rng = np.random.default_rng(100 + n + image_size[0])
    item = _cached_image(rng, n, image_size, (97, 61))
    plan = md.feature_crop_plan(image_size, (32, 24), start=None if image_size == (32, 24) else 3)
    want, K = _reference_cached(item, (32, 24), 32, plan[1])
    L, S, Dm, dp, Kc = ref.feature_pairs_side([item], (32, 24), 32, [plan])
    assert np.array_equal(L[0], want["lafs"]) and np.array_equal(S[0], want["scores"]) and np.array_equal(Dm[0], want["descriptors"])
    assert np.array_equal(dp[0], want["depth"]) and np.array_equal(Kc[0], K)
    if n == 70:
        assert (S[0, :-1] > S[0, 1:]).all()                              # selected: descending


def test_selection_rule_and_outside_depth():
    assert ref.select([1.0, 3.0, 3.0, 0.5, 3.0, 2.0], 4).tolist() == [1, 2, 4, 5]
    assert ref.select([2.0, 2.0, 2.0], 2).tolist() == [0, 1]
    lafs = np.zeros((3, 2, 3), np.float32)
    lafs[:, 0, 2] = [-0.5, 4.0, 1.0]
    lafs[:, 1, 2] = [0.0, 0.0, 3.0]
    depth = np.arange(1, 13, dtype=np.float32).reshape(3, 4)
    out = ref.stack_keypoints(lafs, np.ones(3, np.float32), np.ones((3, 2), np.float32), depth, 5)
    assert out[3].tolist() == [1.0, 0.0, 0.0, 0.0, 0.0]                  # int(-0.5) = 0 is inside; x = 4 and y = 3 are outside: 0


# ---------------------------------------------------------------- the library without a GPU
def test_abi_symbols_are_declared_and_exported():
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "openglue_amd.h")).read()
    declared = set(re.findall(r"^\s*(?:int|size_t)\s+(og_\w+)\s*\(", header, flags=re.M))
    assert NEW_SYMBOLS <= declared and NEW_SYMBOLS <= set(_lib.SYMBOLS)
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
    from openglue_amd import build as og_build
    assert "megadepth.hip" in og_build.SOURCES
    assert ctypes.sizeof(_lib.og_md_frame) == 56 and ctypes.sizeof(_lib.og_md_features) == 88
    for struct in ("og_md_frame", "og_md_features"):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), header, flags=re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body)
        names = [n.strip(" *") for decl in body.split(";") if decl.strip() for n in decl.split(",")]
        names = [n.split()[-1].strip("*") for n in names]
        assert names == [f[0] for f in getattr(_lib, struct)._fields_], names
    assert "og_megadepth_pairs" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def test_entry_points_refuse_before_launching():
    """OG_E_INVALID (-1) for null pointers, OG_E_SHAPE (-2) for sizes and windows, OG_E_ALIGN (-3) for misaligned floats, OG_E_FLAG (-4) for an
    unknown interpolation: all checked before anything is launched (the device addresses are never dereferenced)."""
    lib = _lib.load()
    A = 0x10000
    u8 = lambda **k: lib.og_resize_linear_u8(k.get("B", 1), k.get("H", 8), k.get("W", 9), k.get("C", 3), k.get("src", A), k.get("dw", 12), k.get("dh", 6),
                                             k.get("x0", 0), k.get("y0", 0), k.get("w", 12), k.get("h", 6), k.get("dst", A), None)
    for key in ("src", "dst"):
        assert u8(**{key: None}) == -1, key
    for bad in (dict(C=2), dict(B=0), dict(H=0), dict(W=40000), dict(dw=0), dict(dh=40000), dict(w=0), dict(h=7), dict(x0=1), dict(x0=-1), dict(y0=1), dict(w=13)):
        assert u8(**bad) == -2, bad
    f32 = lambda **k: lib.og_resize_f32(k.get("B", 1), k.get("H", 8), k.get("W", 9), k.get("src", A), k.get("dw", 12), k.get("dh", 6), k.get("nearest", 0),
                                        k.get("x0", 0), k.get("y0", 0), k.get("w", 12), k.get("h", 6), k.get("dst", A), None)
    for key in ("src", "dst"):
        assert f32(**{key: None}) == -1, key
    for bad in (dict(B=0), dict(W=0), dict(dw=0), dict(w=13), dict(y0=1)):
        assert f32(**bad) == -2, bad
    assert f32(nearest=2) == -4 and f32(dst=A + 4) == -3 and f32(src=A + 2) == -3

    def pairs(n=2, tw=32, th=24, host=True, dev=A, images=A, depths=A, K=A, nearest=0, **entry):
        table = (_lib.og_md_frame * 2)()
        for e in table:
            e.image, e.depth, e.K, e.H, e.W, e.C, e.resize_w, e.resize_h, e.x0, e.y0 = A, A, A, 41, 90, 3, 52, 24, 10, 0
        for name, v in entry.items():
            setattr(table[1], name, v)
        return lib.og_megadepth_pairs(n, tw, th, ctypes.addressof(table) if host else None, dev, images, depths, K, nearest, None)
    assert pairs(host=False) == -1
    for key in ("dev", "images", "depths", "K"):
        assert pairs(**{key: None}) == -1, key
    for key in ("image", "depth"):
        assert pairs(**{key: None}) == -1, key
    for bad in (dict(n=0), dict(tw=0), dict(th=0), dict(C=2), dict(H=0), dict(W=40000), dict(resize_w=31), dict(x0=21), dict(x0=-1), dict(y0=1), dict(resize_h=23)):
        assert pairs(**bad) == -2, bad
    assert pairs(nearest=3) == -4 and pairs(images=A + 4) == -3 and pairs(depths=A + 8) == -3 and pairs(depth=A + 2) == -3

    def feats(images=2, tw=32, th=24, k=16, D=8, host=True, dev=A, out=A, **entry):
        table = (_lib.og_md_features * 2)()
        for e in table:
            e.lafs, e.scores, e.descriptors, e.keys, e.depth, e.K = A, A, A, None, A, A
            e.n, e.image_w, e.image_h, e.orig_w, e.orig_h, e.depth_w, e.depth_h, e.axis, e.start = 40, 52, 24, 97, 61, 97, 61, 0, 10
        for name, v in entry.items():
            setattr(table[1], name, v)
        return lib.og_megadepth_features(images, tw, th, k, D, ctypes.addressof(table) if host else None, dev, out, A, A, A, A, None)
    assert feats(host=False) == -1 and feats(dev=None) == -1 and feats(out=None) == -1
    for key in ("lafs", "scores", "descriptors", "depth", "K"):
        assert feats(**{key: None}) == -1, key
    for bad in (dict(images=0), dict(k=0), dict(k=4097), dict(D=0), dict(tw=0)):
        assert feats(**bad) == -2, bad
    for bad in (dict(n=-1), dict(n=8193), dict(image_w=0), dict(depth_h=0), dict(orig_w=40000), dict(axis=2), dict(axis=-2), dict(start=-1), dict(start=21),
                dict(axis=-1), dict(axis=1, start=1)):
        assert feats(**bad) == -2, bad
    assert feats(out=A + 2) == -3 and feats(keys=A + 1) == -3


def test_wrappers_refuse_before_any_device_is_touched():
    u8 = lambda *s: torch.zeros(*s, dtype=torch.uint8)
    f = lambda *s: torch.zeros(*s)
    with pytest.raises(ValueError, match="uint8"):
        md.resize_linear_u8(f(1, 8, 9), (4, 4))
    with pytest.raises(ValueError, match="inside the resized"):
        md.resize_linear_u8(u8(1, 8, 9), (4, 4), (1, 0), (4, 4))
    with pytest.raises(ValueError, match="dsize"):
        md.resize_linear_u8(u8(1, 8, 9), (0, 4))
    with pytest.raises(ValueError, match="float32"):
        md.resize_f32(u8(1, 8, 9), (4, 4))
    with pytest.raises(ValueError, match="'linear' or 'nearest'"):
        md.resize_f32(f(1, 8, 9), (4, 4), "cubic")
    with pytest.raises(ValueError, match=r"\[B, H, W\]"):
        md.resize_f32(f(8, 9), (4, 4))
    K, R, T = f(1, 3, 3), f(1, 3, 3), f(1, 3)
    ok = dict(frames0=[u8(41, 90, 3)], frames1=[u8(53, 37)], depth0=[f(41, 90)], depth1=[f(53, 37)], K0=K, K1=K, R=R, T=T, target_size=(32, 24))
    for change, match in ((dict(frames1=[f(53, 37)]), "uint8"), (dict(frames1=[u8(53, 37, 2)]), "C in"), (dict(depth1=[f(53, 36)]), "frame's size"),
                          (dict(depth0=[]), "same length"), (dict(K1=f(2, 3, 3)), r"K1 must be \[1, 3, 3\]"), (dict(T=f(1, 4)), "T must be"),
                          (dict(depth_interpolation="area"), "'linear' or 'nearest'"), (dict(starts=([0], [99])), "start"),
                          (dict(starts=([0],)), "starts must be"), (dict(target_size=(32,)), "two integers")):
        with pytest.raises(ValueError, match=match):
            md.megadepth_pairs(**{**ok, **change})
    with pytest.raises(RuntimeError, match="GPU"):
        md.megadepth_pairs(**ok)
    with pytest.raises(RuntimeError, match="GPU"):
        md.resize_linear_u8(u8(1, 8, 9), (4, 4))
    item = dict(lafs=f(5, 2, 3), scores=f(5), descriptors=f(5, 8), depth=f(61, 97), K=f(3, 3), image_size=(52, 24), orig_size=(97, 61))
    okf = dict(features0=[item], features1=[item], R=R, T=T, target_size=(32, 24), num_keypoints=16)
    for change, match in ((dict(num_keypoints=0), "num_keypoints"), (dict(num_keypoints=5000), "num_keypoints"), (dict(features1=[]), "same length"),
                          (dict(features1=[{**item, "lafs": f(4, 2, 3)}]), "lafs must be"), (dict(features1=[{**item, "descriptors": f(5, 9)}]), "one D"),
                          (dict(features1=[{**item, "depth": f(3, 61, 97)}]), "depth must be"), (dict(starts=([0], [21])), "start"),
                          (dict(features1=[{**item, "image_size": (52,)}]), "two integers"), (dict(keys=([f(5)],)), "keys must be")):
        with pytest.raises(ValueError, match=match):
            md.megadepth_feature_pairs(**{**okf, **change})
    with pytest.raises(RuntimeError, match="GPU"):
        md.megadepth_feature_pairs(**okf)


def test_megadepth_kernels_use_no_scratch(tmp_path):
    """Every kernel of megadepth.hip compiles for gfx950 without scratch or spills (the figures DESIGN.md 4.15 quotes)"""
    import subprocess
    from openglue_amd import build as og_build
    cmd = [og_build._hipcc(), *og_build.FLAGS, "-Rpass-analysis=kernel-resource-usage", "--cuda-device-only", "-c",
           os.path.join(og_build.CSRC, "megadepth.hip"), "-o", str(tmp_path / "k.o")]
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
    for kernel, instances in (("resize_u8_kernel", 2), ("resize_f32_kernel", 2), ("md_image_kernel", 1), ("md_depth_kernel", 2), ("md_features_kernel", 1)):
        hits = [u for k, u in usage.items() if kernel in k]
        assert len(hits) == instances, (kernel, list(usage))
        for u in hits:
            print(f"{kernel}: SGPRs {u['TotalSGPRs']} VGPRs {u['VGPRs']} scratch {u['ScratchSize [bytes/lane]']} LDS {u['LDS Size [bytes/block]']} "
                  f"occupancy {u['Occupancy [waves/SIMD]']}")
            assert int(u["ScratchSize [bytes/lane]"]) == 0 and int(u["VGPRs Spill"]) == 0 and int(u["SGPRs Spill"]) == 0, (kernel, u)
    assert len(usage) == 8, list(usage)
