"""GPU tests of weak_color_aug (openglue_amd.augment, csrc/coloraug.hip) against the numpy restatement tests/coloraug_ref.py, which
tests/test_coloraug_cpu.py checks on its own.  Equalize, sharpness and solarize are compared bit for bit; the Gaussian noise within a bound
derived from the accuracy of logf / cosf (test_noise).  Small shapes: the whole file takes seconds."""
import numpy as np
import pytest
import torch

from openglue_amd import augment, pairs, supervision, features, synthetic as syn
from tests import coloraug_ref as ref

pytestmark = pytest.mark.gpu
F = np.float32
TX, TY = ref.TILE_X, ref.TILE_Y
# the last one: three histogram blocks per plane, the last of them ragged; 3 x 9 tiles
SHAPES = [(1, 1), (2, 5), (3, 3), (37, 53), (64, 64), (TY - 1, TX - 1), (TY, TX), (TY + 1, TX + 1), (2 * ref.HIST_PIXELS // 129 + 5, 129)]


def _gpu(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _run(image, flags, scalars, seeds, dev, out=None):
    x = image if isinstance(image, torch.Tensor) else _gpu(np.asarray(image, F), dev)
    got = augment.color_aug_packed(x, _gpu(np.asarray(flags, np.int32), dev), _gpu(np.asarray(scalars, F), dev), _gpu(np.asarray(seeds, np.int64), dev), out)
    return got.cpu().numpy()


def _same(a, b):
    return np.array_equal(a, b, equal_nan=True)


def _scalars(B, rng):
    """factor, threshold, addition, mean, std per sample; the factors 0, 1 and 1.5 (the blend's special cases) among them"""
    sc = np.stack([rng.uniform(0, 0.5, B), rng.uniform(0.4, 0.6, B), rng.uniform(-0.1, 0.1, B), np.full(B, 0.01), np.full(B, 0.05)], 1).astype(F)
    sc[2::8, 0], sc[3::8, 0], sc[6::8, 0] = 0.0, 1.0, 1.5
    return sc


@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("H,W", SHAPES)
def test_all_flag_combinations(gpu_device, H, W, C):
    """One call on a batch of 16, sample b with the flags b (every operation alone among them).  Samples b and b + 8 share image and scalars,
    so sample b shows that everything before the noise of sample b + 8 is exact; the noise itself within ref.noise_bound (test_noise)."""
    rng = np.random.default_rng(1000 * H + W + C)
    x8 = rng.random((8, C, H, W), dtype=F)
    x8[1::2] = (rng.integers(0, 256, x8[1::2].shape) / 255.0).astype(F)          # every other image from bytes
    x = np.concatenate([x8, x8])
    sc8 = _scalars(8, rng)
    sc = np.concatenate([sc8, sc8])
    flags, seeds = np.arange(16), rng.integers(0, 2 ** 63 - 1, 16)
    if H * W > ref.HIST_PIXELS:
        assert (H * W + ref.HIST_PIXELS - 1) // ref.HIST_PIXELS >= 3 and H * W % ref.HIST_PIXELS
    got = _run(x, flags, sc, seeds, gpu_device)
    before = ref.color_aug(x, flags, sc, seeds, upto_noise=True)
    want = ref.color_aug(x, flags, sc, seeds)
    assert got.shape == x.shape and got.dtype == F
    for b in range(8):
        assert _same(got[b], want[b]), (b, int((got[b] != want[b]).sum()))
    assert _same(got[0], x[0])                                                  # no flag: a copy
    for b in range(8, 16):
        assert _same(before[b], want[b - 8])
        err = np.abs(got[b].astype(np.float64) - want[b])
        bound = ref.noise_bound(sc[b, 4], sc[b, 3], before[b])
        assert (err <= bound).all(), (b, float(err.max()), float(bound.min()))
        assert (got[b] != before[b]).mean() > 0.5 or H * W < 16                  # the noise is there


def test_noise(gpu_device):
    """The noise stage, out = x + (mean + std z), z = sqrtf(-2 logf(u1)) cosf(6.2831855f u2), against the restatement, whose log and cos are
    float64 rounded to float32 (within half an ulp).  u1, u2 and the argument 6.2831855f u2 are the same floats on both sides.  Assume the
    accurate logf and cosf within 4 ulp (ROCm documents 1-2 ulp for them) and sqrtf correctly rounded (HIP's default).  Then
      l = logf(u1):            |dl| <= 4.5 ulp <= 4.5 * 2^-23 |l|;   -2 l is exact
      s = sqrtf(-2 l):         half the relative error of l, and one rounding on each side: 2.25 * 2^-23 + 2 * 2^-24 = 3.25 * 2^-23
      c = cosf(a):             4.5 * 2^-23 |c|
      z = fl(s c):             3.25 + 4.5 and two roundings: 8.75 * 2^-23, say 9 * 2^-23, relative; |z| <= Z = sqrt(48 ln 2) = 5.77
      n = fl(mean + fl(std z)): |std| Z 9 * 2^-23, and two roundings on each side of values of at most |std| Z and |mean| + |std| Z:
                               |dn| <= (11 |std| Z + |mean|) 2^-23
      out = fl(x + n):         |dn| and one rounding on each side: + 2^-23 (|x| + |mean| + |std| Z)
    which is ref.noise_bound: 5.3e-7 for std 0.05, mean 0, |x| <= 1; a derived number, not one measured on the kernel.
    Then the statistics of the kernel's own z (x = 0, mean 0, std 1 gives z itself) on 256 x 256, the bounds of the CPU test."""
    seeds = np.array([0, 1, 12345, 2 ** 63 - 1], np.int64)
    n = 256 * 256
    zero = np.zeros((4, 1, 256, 256), F)
    sc = np.tile(np.array([0, 0, 0, 0, 1], F), (4, 1))
    z = _run(zero, [8] * 4, sc, seeds, gpu_device)
    for b, seed in enumerate(seeds):
        want = ref.gauss(int(seed), 1, 256, 256)
        err = float(np.abs(z[b].astype(np.float64) - want).max())
        zb = z[b].astype(np.float64).ravel()
        m, s, a = abs(zb.mean()), abs(zb.std() - 1), np.abs(zb).max()
        print(f"seed {seed}: max |z - restatement| {err:.3e} (bound {float(ref.noise_bound(1.0, 0.0, 0.0)):.3e}), |mean| {m:.2e}, |std - 1| {s:.2e}, max |z| {a:.3f}")
        assert err <= ref.noise_bound(1.0, 0.0, 0.0)
        assert m <= 5 / np.sqrt(n) and s <= 5 / np.sqrt(2 * n) and a <= ref.Z_MAX
    # the reference's operating point on an image, three channels: the counter runs on over the channels
    rng = np.random.default_rng(8)
    x = rng.random((2, 3, 37, 53), dtype=F)
    sc = np.tile(np.array([0, 0, 0, 0, 0.05], F), (2, 1))
    got = _run(x, [8, 8], sc, seeds[2:], gpu_device)
    want = ref.color_aug(x, [8, 8], sc, seeds[2:])
    err = np.abs(got.astype(np.float64) - want)
    print(f"std 0.05: max |kernel - restatement| {float(err.max()):.3e}, bound {float(ref.noise_bound(0.05, 0.0, 1.0)):.3e}")
    assert (err <= ref.noise_bound(0.05, 0.0, x)).all()
    assert not np.array_equal(got[0, 0] - x[0, 0], got[0, 1] - x[0, 1])


def test_equalize_edge_cases(gpu_device):
    """the CPU file's edge cases on the device, and a random-float image where histogram bin and table index differ, so that
    (v 256) / 255 must be a true division"""
    sc = np.zeros((1, 5), F)
    for name, img in ref.edge_images().items():
        got = _run(img[None, None], [1], sc, [0], gpu_device)[0, 0]
        want = ref.equalize_plane(img)
        assert _same(got, want), (name, int((got != want).sum()))
        if name == "out_of_range":
            assert np.isfinite(got).all() and got.min() >= 0 and got.max() <= 1
    rng = np.random.default_rng(9)
    x = rng.random((97, 131), dtype=F)
    v = x * F(255)
    assert (ref.to_byte((v * F(256)) / F(255)) != ref.to_byte(v)).sum() > 1000
    got = _run(x[None, None], [1], sc, [0], gpu_device)[0, 0]
    assert _same(got, ref.equalize_plane(x))
    # half the image from values whose bin a multiplication by (float)(1 / 255) gets wrong: the output then differs visibly
    cand = rng.random(1 << 22, dtype=F)
    cv = cand * F(255) * F(256)
    special = cand[ref.to_byte(cv / F(255)) != ref.to_byte(cv * (F(1) / F(255)))]
    assert special.size >= 8
    x.flat[:x.size // 2] = np.resize(special, x.size // 2)
    want = ref.equalize_plane(x)
    assert (want != ref.equalize_plane(x, reciprocal=True)).sum() > 100
    got = _run(x[None, None], [1], sc, [0], gpu_device)[0, 0]
    assert _same(got, want), int((got != want).sum())


def test_determinism_and_batching(gpu_device):
    rng = np.random.default_rng(10)
    B, C, H, W = 5, 3, 45, 67
    x = rng.random((B, C, H, W), dtype=F)
    flags = np.array([15, 9, 0, 7, 14])
    sc, seeds = _scalars(B, rng), rng.integers(0, 2 ** 63 - 1, B)
    xd = _gpu(x, gpu_device)
    out = torch.full_like(xd, float("nan"))
    a = _run(xd, flags, sc, seeds, gpu_device, out)
    assert np.isfinite(a).all()                                                  # every element of the NaN-filled output was written
    assert np.array_equal(xd.cpu().numpy(), x)                                   # the input is unchanged
    b = _run(xd, flags, sc, seeds, gpu_device)
    assert np.array_equal(a, b)                                                  # two runs, the same bits
    for i in range(B):                                                           # a sample alone, with its seed
        one = _run(x[i:i + 1], flags[i:i + 1], sc[i:i + 1], seeds[i:i + 1], gpu_device)
        assert np.array_equal(one[0], a[i]), i
    # the public wrapper: a non-contiguous view gives what its contiguous copy gives
    params = {"equalize": flags & 1, "sharpness": flags & 2, "solarize": flags & 4, "noise": flags & 8}
    params = {k: _gpu(v.astype(bool), gpu_device) for k, v in params.items()}
    params.update({k: _gpu(sc[:, i], gpu_device) for i, k in enumerate(("factor", "threshold", "addition", "noise_mean", "noise_std"))})
    params["seed"] = _gpu(seeds.astype(np.int64), gpu_device)
    assert np.array_equal(augment.color_aug(xd, params).cpu().numpy(), a)
    wide = _gpu(np.concatenate([x, x[..., ::-1]], axis=3), gpu_device)
    view = wide[..., :W]
    assert not view.is_contiguous()
    assert np.array_equal(augment.color_aug(view, params).cpu().numpy(), a)
    assert np.array_equal(augment.color_aug(xd.permute(0, 1, 3, 2), params).cpu().numpy(),
                          augment.color_aug(xd.permute(0, 1, 3, 2).contiguous(), params).cpu().numpy())


def test_sampler_on_the_device(gpu_device):
    gen = lambda s: torch.Generator(device=gpu_device).manual_seed(s)
    p, q, r = (augment.sample_weak_color_aug(512, gpu_device, gen(s)) for s in (3, 3, 4))
    assert all(v.device.type == "cuda" for v in p.values())
    assert all(torch.equal(p[k], q[k]) for k in p) and not torch.equal(p["seed"], r["seed"])
    assert 0.15 < float(p["equalize"].float().mean()) < 0.35 and 0.4 < float(p["noise"].float().mean()) < 0.6     # 5 sigma at 512 draws
    assert float(p["factor"].min()) >= 0 and float(p["factor"].max()) <= 0.5 and int(p["seed"].min()) >= 0


def test_augment_on_a_pair_item(gpu_device):
    """MatchingTrainingModule.augment on homography_pairs items: every sample is what color_aug makes of it with the draw of the same
    generator state, changed exactly where a flag was drawn; H is untouched; generate_gt_matches takes the item as before."""
    t = augment.get_augmentation_transform({"name": "weak_color_aug"})
    gen = lambda s: torch.Generator(device=gpu_device).manual_seed(s)
    frames = torch.randint(0, 256, (8, 80, 96, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(0)).to(gpu_device)
    item = pairs.homography_pairs(frames, 12, generator=gen(1))
    image0, image1, Hm = item["image0"], item["image1"], item["transformation"]["H"].clone()
    out = augment.augment(item, t, gen(2))
    assert out is item and torch.equal(out["transformation"]["H"], Hm) and out["transformation"]["type"] == ["perspective"] * 8
    g = gen(2)
    flagged = 0
    for key, orig in (("image0", image0), ("image1", image1)):
        params = augment.sample_weak_color_aug(8, gpu_device, g)
        assert out[key] is not orig and torch.equal(out[key], augment.color_aug(orig, params))
        on = (params["equalize"] | params["sharpness"] | params["solarize"] | params["noise"]).cpu()
        changed = (out[key] != orig).flatten(1).any(1).cpu()
        assert torch.equal(on, changed)
        flagged += int(on.sum())
    assert flagged > 0                                                           # 16 draws, each unflagged with probability 0.21
    assert augment.augment({"image0": image0, "image1": image1, "transformation": {}}, augment.get_augmentation_transform({"name": "none"}))["image0"] is image0
    # one 240 x 320 pair through the extractor into the labels
    from openglue_amd.sift import SIFT
    rgb = torch.cat([syn.make_image(240, 320, seed=51 + c) for c in range(3)], dim=1)
    frame = (rgb * 255).round().to(torch.uint8).permute(0, 2, 3, 1).contiguous().to(gpu_device)
    wo = torch.tensor([[[10, -7], [-12, 9], [-5, -20], [14, 6]]], dtype=torch.float32, device=gpu_device)
    data = augment.augment(pairs.homography_pairs(frame, 24, wo), t, gen(5))
    net = SIFT(max_keypoints=256)
    f = [features.prepare_features_output(*net(data[k]), "none") for k in ("image0", "image1")]
    merged, y = supervision.generate_gt_matches(data, f[0], f[1], 3.0)
    assert merged is not None and merged["image0"] is data["image0"]
    assert y["gt_matches0"].shape == (1, f[0]["keypoints"].shape[1]) and int((y["gt_matches0"] >= 0).sum()) > 0
