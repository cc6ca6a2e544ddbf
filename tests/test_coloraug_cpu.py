"""CPU checks of weak_color_aug (openglue_amd.augment, og_color_aug_workspace_bytes / og_color_aug): the numpy restatement in
tests/coloraug_ref.py against the ATen formulation of kornia's functions beside it, so that the GPU tests compare against something known
to be right; the equalize edge cases; the statistics of the counter-based noise; the refusals; the ABI; the sampler; the compiled kernels'
resources.  No kernel is launched here."""
import os
import re

import numpy as np
import pytest
import torch

from openglue_amd import _lib
from tests import coloraug_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = {"og_color_aug_workspace_bytes", "og_color_aug"}
SIZES = [(1, 1), (2, 5), (37, 53), (64, 64)]
F = np.float32


def _byte_image(H, W, seed):
    return (np.random.default_rng(seed).integers(0, 256, (H, W)) / 255.0).astype(F)


def _float_image(H, W, seed):
    return np.random.default_rng(seed).random((H, W), dtype=F)


# ---------------------------------------------------------------- restatement against the ATen formulation
def test_bytes_survive_the_round_trip():
    k = np.arange(256)
    assert np.array_equal((k / 255.0).astype(F) * F(255), k.astype(F))


@pytest.mark.parametrize("H,W", SIZES)
@pytest.mark.parametrize("kind", ["bytes", "floats"])
def test_equalize_equals_aten(H, W, kind):
    for seed in range(3):
        x = (_byte_image if kind == "bytes" else _float_image)(H, W, 10 * H + seed)
        want = ref.aten_equalize_plane(torch.from_numpy(x)).numpy()
        got = ref.equalize_plane(x)
        assert got.dtype == F and np.array_equal(got, want), (kind, H, W, seed, int((got != want).sum()))


@pytest.mark.parametrize("H,W", SIZES)
def test_solarize_equals_aten(H, W):
    rng = np.random.default_rng(H)
    for kind in (_byte_image, _float_image):
        x = np.stack([kind(H, W, s) for s in range(4)])[:, None]
        thr = rng.uniform(0.4, 0.6, 4).astype(F)
        add = rng.uniform(-0.1, 0.1, 4).astype(F)
        want = ref.aten_solarize(torch.from_numpy(x), torch.from_numpy(thr), torch.from_numpy(add)).numpy()
        got = np.stack([ref.solarize_plane(x[b, 0], thr[b], add[b]) for b in range(4)])[:, None]
        assert np.array_equal(got, want)
        assert (got != x).any()


@pytest.mark.parametrize("H,W", SIZES + [(3, 3)])
def test_sharpness_agrees_with_aten(H, W):
    """The restatement fixes the order of the nine products and eight sums; conv2d's order is its own.  Both are float32 evaluations of
    one sum of nine non-negative terms w_i x_i with sum w_i = 1 (up to the rounding of 1/13 and 5/13) and x_i in [0, 1]: every partial sum
    is at most 1 + O(2^-23), so each of the nine products and eight sums of either evaluation errs by at most half an ulp of 1,
    2^-24, and the two blurs differ by at most 2 * 17 * 2^-24 (the issue's 2 * 9 * 2^-24 counts the terms, this counts every rounding).
    The clamp moves them no further apart.  The blend blur + (in - blur) f with |f| <= 2 is the same three operations on both sides; a
    difference d of the blurs passes through as at most |1 - f| d + |f| d <= 3 d, plus three roundings of values of at most 3 on
    each side, 2 * 3 * 2^-23.  Bound: 3 * 34 * 2^-24 + 6 * 2^-23 = 114 * 2^-24 = 6.8e-6 (for 0 <= f <= 1, where the blend is a convex
    combination, a third of that)."""
    if H < 3 or W < 3:
        x = _float_image(H, W, 1)
        assert np.array_equal(ref.sharpness_plane(x, 0.3), x)          # every pixel is a border pixel (kornia's conv2d would raise)
        return
    bound = 114 * 2.0 ** -24
    worst = 0.0
    for kind in (_byte_image, _float_image):
        x = np.stack([kind(H, W, 20 + s) for s in range(6)])[:, None]
        f = np.array([0.0, 1.0, 0.25, 0.4999, 1.5, 2.0], F)
        want = ref.aten_sharpness(torch.from_numpy(x), torch.from_numpy(f)).numpy()
        got = np.stack([ref.sharpness_plane(x[b, 0], f[b]) for b in range(6)])[:, None]
        assert np.array_equal(got[1], x[1])                             # f == 1: the input
        edge = np.ones((H, W), bool)
        edge[1:-1, 1:-1] = False
        assert np.array_equal(got[:, 0][:, edge], x[:, 0][:, edge])       # the border keeps the input
        worst = max(worst, float(np.abs(got - want).max()))
    print(f"{H} x {W}: max |restatement - conv2d formulation| {worst:.3e}, bound {bound:.3e}")
    assert worst <= bound


# ---------------------------------------------------------------- equalize edge cases
def test_equalize_edge_cases():
    im = ref.edge_images()
    c = im["constant"]
    assert np.array_equal(ref.equalize_plane(c), (c * F(255)) / F(255))
    t = ref.equalize_plane(im["two_level"])
    # N = 1024, last bin 512: step = 2; lut[200] = (512 + 1) // 2 = 256 -> 255; lut[0] = 0
    assert set(np.unique(t)) == {F(0), F(1)} and np.array_equal(t == 1, im["two_level"] > 0)
    b = im["last_bin_all_but_254"]
    assert (1600 - (1600 - 254)) // 255 == 0 and np.array_equal(ref.equalize_plane(b), (b * F(255)) / F(255))
    o = ref.equalize_plane(im["ones"])
    assert np.array_equal(o, ref.aten_equalize_plane(torch.from_numpy(im["ones"])).numpy()) and o.max() == 1
    w = ref.equalize_plane(im["out_of_range"])                              # step != 0: everything goes through the table
    assert np.isfinite(w).all() and w.min() >= 0 and w.max() <= 1
    assert w[0, 0] == w[0, 2] == w[0, 3] == 0 and w[0, 1] == 1              # NaN and negatives: entry 0; +inf: entry 255
    inside = (im["out_of_range"] >= 0) & (im["out_of_range"] <= 1)
    assert inside.sum() > 300


# ---------------------------------------------------------------- the noise
@pytest.mark.parametrize("seed", [0, 1, 12345, 2 ** 63 - 1])
def test_noise_statistics(seed):
    z = ref.gauss(seed, 1, 256, 256).astype(np.float64).ravel()
    n = z.size
    m, s, a = abs(z.mean()), abs(z.std() - 1), np.abs(z).max()
    print(f"seed {seed}: |mean| {m:.2e} (bound {5 / np.sqrt(n):.2e}), |std - 1| {s:.2e} (bound {5 / np.sqrt(2 * n):.2e}), max |z| {a:.3f} (bound {ref.Z_MAX:.3f})")
    assert m <= 5 / np.sqrt(n) and s <= 5 / np.sqrt(2 * n) and a <= ref.Z_MAX


def test_noise_is_counter_based():
    """sample b of a batch equals the sample alone; channel c of a 3-channel sample continues the counter at c H W"""
    z = ref.gauss(7, 3, 5, 6)
    i = np.arange(90, dtype=np.uint64)
    with np.errstate(over="ignore"):
        h = ref.mix64(ref.mix64(np.array([7], np.uint64)) + i)
    assert h.dtype == np.uint64 and len(set(h.tolist())) == 90
    assert ref.mix64(np.array([0], np.uint64))[0] == 0xE220A8397B1DCDAF       # splitmix64's first output for state 0
    x = np.zeros((3, 5, 6), F)
    assert np.array_equal(ref.noise_sample(x, 7, 0.0, 1.0), z)


def test_color_aug_order_and_copy():
    rng = np.random.default_rng(3)
    x = rng.random((16, 1, 12, 13), dtype=F)
    flags = np.arange(16)
    sc = np.tile(np.array([0.3, 0.55, 0.05, 0.0, 0.05], F), (16, 1))
    seeds = np.arange(16) + 100
    out = ref.color_aug(x, flags, sc, seeds)
    assert np.array_equal(out[0], x[0])                                         # no flag: a copy
    want = ref.noise_sample(ref.solarize_plane(ref.sharpness_plane(ref.equalize_plane(x[15, 0]), 0.3), 0.55, 0.05)[None], 115, 0.0, 0.05)
    assert np.array_equal(out[15], want)
    assert all((out[b] != x[b]).any() for b in range(1, 16))


# ---------------------------------------------------------------- ABI, refusals, sampler
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
    assert "coloraug.hip" in og_build.SOURCES
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert all(name in integration for name in NEW_SYMBOLS)


def test_workspace_bytes():
    lib = _lib.load()
    nblk = lambda n: (n + ref.HIST_PIXELS - 1) // ref.HIST_PIXELS
    for B, C, H, W in ((1, 1, 1, 1), (4, 1, 720, 960), (2, 3, 37, 53), (65535, 3, 8, 8)):
        need = B * C * (nblk(H * W) * 1024 + 1024 + 4)
        got = lib.og_color_aug_workspace_bytes(B, C, H, W)
        assert need <= got < need + 256 and got % 256 == 0
    for bad in ((0, 1, 8, 8), (1, 2, 8, 8), (1, 1, 0, 8), (1, 1, 8, 32769), (65536, 1, 8, 8)):
        assert lib.og_color_aug_workspace_bytes(*bad) == 0


def test_entry_point_refuses_before_launching():
    """OG_E_INVALID (-1) for a null pointer or dst == src, OG_E_SHAPE (-2) for the sizes and a short workspace, OG_E_ALIGN (-3) for
    misaligned tables: all checked before anything is launched (the addresses are never dereferenced)."""
    lib = _lib.load()
    A = 0x10000
    big = 1 << 30
    aug = lambda **k: lib.og_color_aug(k.get("B", 2), k.get("C", 1), k.get("H", 8), k.get("W", 9), k.get("src", A), k.get("dst", 2 * A), k.get("flags", A),
                                       k.get("scalars", A), k.get("seeds", A), k.get("ws", A), k.get("bytes", big), None)
    for key in ("src", "dst", "flags", "scalars", "seeds", "ws"):
        assert aug(**{key: None}) == -1, key
    assert aug(dst=A) == -1
    for bad in (dict(C=2), dict(C=0), dict(C=4), dict(B=0), dict(B=65536), dict(H=0), dict(W=0), dict(H=32769), dict(W=40000), dict(bytes=0),
                dict(bytes=lib.og_color_aug_workspace_bytes(2, 1, 8, 9) - 1)):
        assert aug(**bad) == -2, bad
    for key, off in (("flags", 2), ("scalars", 2), ("seeds", 4), ("ws", 1), ("src", 2), ("dst", 2)):
        assert aug(**{key: (2 * A if key == "dst" else A) + off}) == -3, key


def _params(B):
    z = lambda dtype: torch.zeros(B, dtype=dtype)
    return {**{k: z(torch.bool) for k in ("equalize", "sharpness", "solarize", "noise")},
            **{k: z(torch.float32) for k in ("factor", "threshold", "addition", "noise_mean", "noise_std")}, "seed": z(torch.int64)}


def test_wrappers_refuse_before_any_device_is_touched():
    from openglue_amd import augment
    img = torch.zeros(2, 1, 8, 8)
    with pytest.raises(ValueError, match=r"\[B, C, H, W\]"):
        augment.color_aug(torch.zeros(2, 8, 8), _params(2))
    with pytest.raises(ValueError, match=r"C in"):
        augment.color_aug(torch.zeros(2, 2, 8, 8), _params(2))
    with pytest.raises(ValueError, match="float32"):
        augment.color_aug(img.double(), _params(2))
    with pytest.raises(ValueError, match="0 < B"):
        augment.color_aug(torch.zeros(0, 1, 8, 8), _params(2))
    with pytest.raises(ValueError, match="dictionary"):
        augment.color_aug(img, None)
    with pytest.raises(ValueError, match="lacks 'seed'"):
        augment.color_aug(img, {k: v for k, v in _params(2).items() if k != "seed"})
    with pytest.raises(ValueError, match=r"params\['factor'\]"):
        augment.color_aug(img, {**_params(2), "factor": torch.zeros(3)})
    with pytest.raises(ValueError, match=r"params\['equalize'\]"):
        augment.color_aug(img, {**_params(2), "equalize": torch.zeros(2)})
    with pytest.raises(ValueError, match=r"params\['seed'\]"):
        augment.color_aug(img, {**_params(2), "seed": torch.zeros(2, dtype=torch.int32)})
    with pytest.raises(ValueError, match="batch must be"):
        augment.sample_weak_color_aug(0, "cpu")
    with pytest.raises(ValueError, match="probabilities"):
        augment.sample_weak_color_aug(2, "cpu", p_noise=1.5)
    # well-formed arguments that are not on the GPU: the library has no CPU path
    with pytest.raises(RuntimeError, match="GPU"):
        augment.color_aug(img, _params(2))
    with pytest.raises(NameError, match="strong_aug module was not found"):
        augment.get_augmentation_transform({"name": "strong_aug"})


def test_none_is_the_identity_and_augment_uses_it():
    from openglue_amd import augment
    t = augment.get_augmentation_transform({"name": "none"})
    assert t.transform_matrix is None
    img = torch.rand(2, 1, 8, 8)
    assert t(img) is img and t(img, None) is img
    K = torch.eye(3).repeat(2, 1, 1)
    batch = {"image0": img, "image1": img + 1, "transformation": {"K0": K, "K1": K, "type": ["3d_reprojection"] * 2}}
    out = augment.augment(batch, t)
    assert out is batch and out["image0"] is img and out["transformation"]["K0"] is K and out["transformation"]["K1"] is K
    assert augment.get_augmentation_transform({"name": "weak_color_aug"}).transform_matrix is None


def test_sampler_ranges_and_frequencies():
    """4096 draws on the CPU generator (the code path is the device's): every flag frequency within 5 sigma of its binomial expectation,
    sigma = sqrt(p (1 - p) / n); the scalars inside their intervals, and spread over them (mean within 5 sigma of the uniform's)."""
    from openglue_amd import augment
    n = 4096
    g = torch.Generator().manual_seed(0)
    p = augment.sample_weak_color_aug(n, "cpu", g)
    for name, prob in (("equalize", .25), ("sharpness", .25), ("solarize", .25), ("noise", .5)):
        assert p[name].dtype == torch.bool and p[name].shape == (n,)
        freq = float(p[name].float().mean())
        assert abs(freq - prob) <= 5 * np.sqrt(prob * (1 - prob) / n), (name, freq)
    for name, lo, hi in (("factor", 0.0, 0.5), ("threshold", 0.4, 0.6), ("addition", -0.1, 0.1)):
        v = p[name]
        assert v.dtype == torch.float32 and v.shape == (n,) and float(v.min()) >= lo - 1e-7 and float(v.max()) <= hi + 1e-7
        assert abs(float(v.mean()) - (lo + hi) / 2) <= 5 * (hi - lo) / np.sqrt(12 * n), name
    assert torch.equal(p["noise_mean"], torch.zeros(n)) and torch.equal(p["noise_std"], torch.full((n,), 0.05))
    assert p["seed"].dtype == torch.int64 and int(p["seed"].min()) >= 0 and len(set(p["seed"].tolist())) == n
    flags, scalars, seeds = augment.pack_params(p)
    assert flags.dtype == torch.int32 and scalars.shape == (n, 5) and scalars.is_contiguous() and seeds is not None
    want = p["equalize"].int() + 2 * p["sharpness"].int() + 4 * p["solarize"].int() + 8 * p["noise"].int()
    assert torch.equal(flags, want.to(torch.int32)) and torch.equal(scalars[:, 1], p["threshold"])
    q = augment.sample_weak_color_aug(n, "cpu", torch.Generator().manual_seed(0))
    assert all(torch.equal(p[k], q[k]) for k in p)
    r = augment.sample_weak_color_aug(64, "cpu", g, p_equalize=1.0, p_sharpness=0.0, p_solarize=1.0, p_noise=0.0, noise_std=0.1, sharpness=1.0)
    assert bool(r["equalize"].all()) and not bool(r["sharpness"].any()) and bool(r["solarize"].all()) and not bool(r["noise"].any())
    assert torch.equal(r["noise_std"], torch.full((64,), 0.1))


# ---------------------------------------------------------------- build
def test_coloraug_kernels_use_no_scratch(tmp_path):
    """Every kernel of coloraug.hip compiles for gfx950 without scratch or spills and keeps eight waves per SIMD."""
    import subprocess
    from openglue_amd import build as og_build
    cmd = [og_build._hipcc(), *og_build.FLAGS, "-Rpass-analysis=kernel-resource-usage", "--cuda-device-only", "-c",
           os.path.join(og_build.CSRC, "coloraug.hip"), "-o", str(tmp_path / "k.o")]
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
    for kernel in ("coloraug_hist_kernel", "coloraug_lut_kernel", "coloraug_apply_kernel"):
        hits = [u for k, u in usage.items() if kernel in k]
        assert len(hits) == 1, (kernel, list(usage))
        u = hits[0]
        print(f"{kernel}: SGPRs {u['TotalSGPRs']} VGPRs {u['VGPRs']} scratch {u['ScratchSize [bytes/lane]']} LDS {u['LDS Size [bytes/block]']} "
              f"occupancy {u['Occupancy [waves/SIMD]']}")
        assert int(u["ScratchSize [bytes/lane]"]) == 0 and int(u["VGPRs Spill"]) == 0 and int(u["SGPRs Spill"]) == 0, (kernel, u)
        assert int(u["Occupancy [waves/SIMD]"]) >= 8, (kernel, u)
    assert len(usage) == 3, list(usage)
    src = open(os.path.join(og_build.CSRC, "coloraug.hip")).read()
    assert f"kTileX = {ref.TILE_X}, kTileY = {ref.TILE_Y}" in src and f"kHistPixels = {ref.HIST_PIXELS};" in src      # the GPU tests' shapes follow these
    assert "-ffast-math" not in " ".join(og_build.FLAGS + og_build.PER_FILE_FLAGS.get("coloraug.hip", []))
