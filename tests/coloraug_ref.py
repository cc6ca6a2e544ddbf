"""The specification of weak_color_aug (openglue_amd.augment, og_color_aug, csrc/coloraug.hip) restated in numpy, and beside it the ATen
formulation of kornia's four functions (enhance.equalize, enhance.sharpness, enhance.solarize, RandomGaussianNoise) in torch operators,
against which tests/test_coloraug_cpu.py checks the restatement.  kornia itself is not a dependency of the tests: the aten_* functions
follow its code line by line (kornia/enhance/adjust.py: _scale_channel, _build_lut, sharpness, _blend_one, solarize).

Everything is float32 with every operation rounded on its own; numpy's float32 arithmetic is exactly that."""
import numpy as np
import torch

F = np.float32
EQUALIZE, SHARPNESS, SOLARIZE, NOISE = 1, 2, 4, 8
TILE_X, TILE_Y = 64, 16              # kTileX, kTileY of csrc/coloraug.hip
HIST_PIXELS = 8192                   # kHistPixels of csrc/coloraug.hip: pixels of a plane per histogram block
Z_MAX = float(np.sqrt(48 * np.log(2)))      # u1 >= 2^-24: |z| <= sqrt(-2 ln 2^-24)


def to_byte(q):
    """q >= 255 ? 255 : q >= 0 ? (int)q : 0; a NaN gives 0"""
    with np.errstate(invalid="ignore"):
        q = np.where(q >= 0, q, F(0))                     # NaN and negatives
        return np.minimum(q, F(255)).astype(np.int64)     # truncation


def equalize_plane(x, reciprocal=False):
    """one [H, W] float32 plane.  reciprocal: the WRONG bin formula, v 256 times (float)(1 / 255) in place of the division, for the test that
    shows a kernel doing so would be caught"""
    x = np.asarray(x, F)
    v = x * F(255)
    with np.errstate(over="ignore", invalid="ignore"):
        b = to_byte((v * F(256)) * (F(1) / F(255)) if reciprocal else (v * F(256)) / F(255))
    idx = to_byte(v)
    h = np.bincount(b.ravel(), minlength=256).astype(np.int64)
    last = int(np.nonzero(h)[0][-1])
    step = (x.size - int(h[last])) // 255
    if step == 0:
        return v / F(255)
    cum = np.cumsum(h)
    lut = np.zeros(256, np.int64)
    lut[1:] = np.clip((cum[:-1] + step // 2) // step, 0, 255)
    return (lut.astype(F) / F(255))[idx]


def clamp01(t):
    with np.errstate(invalid="ignore"):
        return np.where(t < 0, F(0), np.where(t > 1, F(1), t)).astype(F)


def sharpness_plane(x, f):
    x = np.asarray(x, F)
    f = F(f)
    H, W = x.shape
    out = x.copy()
    if H < 3 or W < 3:
        return out
    w1, w5 = F(1) / F(13), F(5) / F(13)
    acc = None
    for dy in range(3):
        for dx in range(3):
            term = (w5 if dy == dx == 1 else w1) * x[dy:H - 2 + dy, dx:W - 2 + dx]
            acc = term if acc is None else acc + term
    blur = clamp01(acc)
    inner = x[1:-1, 1:-1]
    if f == 0:
        r = blur
    elif f == 1:
        r = inner
    else:
        r = blur + (inner - blur) * f
        if not (0 < f < 1):
            r = clamp01(r)
    out[1:-1, 1:-1] = r
    return out


def solarize_plane(x, threshold, addition):
    t = clamp01(np.asarray(x, F) + F(addition))
    with np.errstate(invalid="ignore"):
        return np.where(t < F(threshold), t, F(1) - t).astype(F)


def mix64(z):
    """csrc/og_ransac.h:29 on uint64 arrays, wrapping"""
    z = np.asarray(z, np.uint64)
    with np.errstate(over="ignore"):
        z = z + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def gauss(seed, C, H, W):
    """z [C, H, W] float32 of one sample; log and cos in float64, rounded"""
    i = np.arange(C * H * W, dtype=np.uint64)
    with np.errstate(over="ignore"):
        h = mix64(mix64(np.array([seed], np.uint64)) + i)
    u1 = ((h >> np.uint64(40)) + np.uint64(1)).astype(F) * F(2.0 ** -24)
    u2 = ((h >> np.uint64(16)) & np.uint64(0xFFFFFF)).astype(F) * F(2.0 ** -24)
    l = np.log(u1.astype(np.float64)).astype(F)
    s = np.sqrt((F(-2) * l).astype(np.float64)).astype(F)
    c = np.cos((F(6.2831855) * u2).astype(np.float64)).astype(F)
    return (s * c).reshape(C, H, W)


def noise_sample(x, seed, mean, std):
    x = np.asarray(x, F)
    return x + (F(mean) + F(std) * gauss(seed, *x.shape))


def color_aug(image, flags, scalars, seeds, upto_noise=False):
    """image [B, C, H, W] float32, flags [B], scalars [B, 5], seeds [B] -> the augmented batch; upto_noise: the input of the noise stage"""
    image = np.asarray(image, F)
    out = image.copy()
    for b in range(image.shape[0]):
        fl = int(flags[b])
        factor, threshold, addition, mean, std = (F(v) for v in scalars[b])
        s = image[b].copy()
        if fl & EQUALIZE:
            s = np.stack([equalize_plane(p) for p in s])
        if fl & SHARPNESS:
            s = np.stack([sharpness_plane(p, factor) for p in s])
        if fl & SOLARIZE:
            s = np.stack([solarize_plane(p, threshold, addition) for p in s])
        if fl & NOISE and not upto_noise:
            s = noise_sample(s, int(seeds[b]), mean, std)
        out[b] = s
    return out


def noise_bound(std, mean, x):
    """|kernel - restatement| of the noise stage on the same input x (tests/test_gpu_coloraug.py derives it)"""
    e = 2.0 ** -23
    return (abs(std) * Z_MAX * 11 + abs(mean)) * e + e * (np.abs(x) + abs(mean) + abs(std) * Z_MAX)


def edge_images():
    """name -> [H, W] float32 plane; the equalize edge cases of the CPU and the GPU tests"""
    out = {}
    out["constant"] = np.full((9, 11), 0.3, F)                              # one bin: step == 0
    two = np.zeros((32, 32), F)
    two[:, 16:] = F(200 / 255)
    out["two_level"] = two
    big = np.full((40, 40), F(254 / 255), F)                              # the last non-empty bin holds all but 254 pixels: step == 0
    big.flat[:254] = (np.arange(254) / 255.0).astype(F)
    out["last_bin_all_but_254"] = big
    ones = (np.random.default_rng(5).integers(0, 256, (24, 24)) / 255.0).astype(F)
    ones[::3] = F(1.0)                                                      # v = 255: histc's bin 256 becomes 255
    out["ones"] = ones
    wild = np.random.default_rng(6).random((24, 24), dtype=F) * F(1.4) - F(0.2)
    wild[0, :4] = [np.nan, np.inf, -np.inf, -5.0]
    out["out_of_range"] = wild
    return out


# ---------------------------------------------------------------- kornia's functions in ATen operators
def aten_equalize_plane(im):
    """kornia.enhance.equalize -> _scale_channel on one [H, W] plane (without its range check, which raises)"""
    im = im * 255.0
    histo = torch.histc(im, bins=256, min=0, max=255)
    nonzero_histo = torch.reshape(histo[histo != 0], [-1])
    step = (torch.sum(nonzero_histo) - nonzero_histo[-1]) // 255
    if step == 0:
        result = im
    else:
        step_trunc = torch.div(step, 2, rounding_mode="trunc")
        lut = torch.div(torch.cumsum(histo, 0) + step_trunc, step, rounding_mode="trunc")
        lut = torch.cat([torch.zeros(1, dtype=lut.dtype), lut[:-1]])
        lut = torch.clamp(lut, 0, 255)
        result = torch.gather(lut, 0, im.flatten().long()).reshape_as(im)
    return result / 255.0


def aten_sharpness(x, factor):
    """kornia.enhance.sharpness on [B, C, H, W] with one factor per sample"""
    C = x.shape[1]
    kernel = torch.tensor([[1, 1, 1], [1, 5, 1], [1, 1, 1]], dtype=x.dtype).view(1, 1, 3, 3).repeat(C, 1, 1, 1) / 13
    degenerate = torch.nn.functional.conv2d(x, kernel, bias=None, stride=1, groups=C)
    degenerate = torch.clamp(degenerate, 0.0, 1.0)
    mask = torch.ones_like(degenerate)
    padded_mask = torch.nn.functional.pad(mask, [1, 1, 1, 1])
    padded_degenerate = torch.nn.functional.pad(degenerate, [1, 1, 1, 1])
    result = torch.where(padded_mask == 1, padded_degenerate, x)

    def blend(input1, input2, f):
        if f == 0.0:
            return input1
        if f == 1.0:
            return input2
        res = input1 + (input2 - input1) * f
        if 0.0 < f < 1.0:
            return res
        return torch.clamp(res, 0, 1)
    return torch.stack([blend(result[i], x[i], factor[i]) for i in range(len(factor))])


def aten_solarize(x, thresholds, additions):
    """kornia.enhance.solarize on [B, C, H, W] with one threshold and one addition per sample"""
    x = torch.clamp(x + additions.view(-1, 1, 1, 1), 0.0, 1.0)
    return torch.where(x < thresholds.view(-1, 1, 1, 1), x, 1.0 - x)
