"""Crafted inputs for the stage-level tests of the DoG + AffNet + OriNet + HardNet extractor (csrc/patchnet.hip: pn_blur_kernel /
pn_resize_kernel, pn_extract_kernel, the trunk, the two tails and the LAF updates).  tests/test_patchnet_cases_cpu.py proves on the
CPU, with the float64 restatement (tests/patchnet_ref.py), that every case reaches the edge it names; tests/test_gpu_patchnet_stages.py
feeds the same tensors to og_patch_pyramid / og_patch_extract / og_patchnet_forward and holds the kernels to the restatement.

torch on the CPU only, deterministic (seeded generators).  A case that claims an exact answer carries the closed form (`closed`,
`exact_levels`): the CPU test proves that the float32 and the float64 restatement both equal it bit for bit (e32 == 0), and only then
does the GPU test ask for equality.  Why those are exact in fp32:
  pyramid   constants c in {1, 2, 3} at even sizes: the blur's partial sums are c times an integer <= 256, the resize weights are
            exactly 0.5; constants 1, 2, 4 at odd sizes: (1 - l) + l rounds to 1 for every fp32 l in [0, 1).  Integer images 0..63 at
            even sizes: every partial sum of level 1 is an integer / 2^18 below 2^24.
  extract   a LAF 16 M with M a signed permutation and an integer centre puts every sample on a pixel: the weights are 0 and 1.
            The restatement samples through grid_sample, whose round trip p -> (2 p + 1) / size - 1 -> p loses the last bits of p
            near 0 when the size is no power of two; the crops over the top border therefore sit on a 64 x 128 image (crops-pow2),
            and the same LAFs at height 96 are held to the tolerance rule instead (clamp-top-96).
  networks  a dead trunk with a zero tail mean gives 0 / 1e-12 = 0 in every precision.
"""
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Tuple

import torch

PS = 32
CHUNK = 512                  # PN_CHUNK of the source: patches per pass through the trunk
WIDTH = {"hardnet": 128, "affnet": 3, "orinet": 2}
SENTINEL = -777.25           # what the rows behind n hold before and after a call
EXTRA = 8                    # sentinel rows behind n


def rand_image(B, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(B, 1, H, W, generator=g)


def ramp(H, W):
    """3 x + 5 y: a plane, which a bilinear resize samples without error and the blur leaves alone away from the border"""
    y, x = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    return (3.0 * x + 5.0 * y)[None, None]


# ---------------------------------------------------------------- pyramid
@dataclass
class PyramidCase:
    name: str
    image: torch.Tensor                               # [B, 1, H, W] float32
    sizes: List[Tuple[int, int]]                      # the levels that are built
    edge: str
    exact_levels: Tuple[int, ...] = (0,)              # levels whose fp32 restatement is proved bit-equal to float64 (level 0 is a copy)
    constant: bool = False                            # every level of image b is image[b, 0, 0, 0]
    is_ramp: bool = False


SIZES = {(32, 32): [(32, 32)], (63, 90): [(63, 90)], (64, 64): [(64, 64), (32, 32)], (65, 67): [(65, 67), (32, 33)],
         (97, 131): [(97, 131), (48, 65)], (128, 160): [(128, 160), (64, 80), (32, 40)], (160, 96): [(160, 96), (80, 48)]}
IMPULSES_64 = [(0, 0), (0, 1), (1, 0), (63, 63), (62, 63), (20, 37)]


def pyramid_cases():
    out = []
    edges = {(32, 32): "one level: the copy alone, no blur or resize launch", (63, 90): "one level, odd side just below 64",
             (64, 64): "the last level is exactly 32 x 32", (65, 67): "odd sides: resize ratios 65 / 32 and 67 / 33, neither is 2",
             (97, 131): "odd sides, ratios 97 / 48 and 131 / 65", (128, 160): "three levels", (160, 96): "portrait"}
    for k, ((H, W), sizes) in enumerate(SIZES.items()):
        out.append(PyramidCase(f"random-{H}x{W}", rand_image(1, H, W, 300 + k), sizes, edges[(H, W)]))
    out.append(PyramidCase("batch3-65x67", rand_image(3, 65, 67, 320), SIZES[(65, 67)], "B = 3, three different images, odd sides"))
    const = torch.arange(1, 4, dtype=torch.float32).view(3, 1, 1, 1)
    out.append(PyramidCase("constant-b+1-128x160", const.expand(3, 1, 128, 160).contiguous(), SIZES[(128, 160)],
                           "image b is b + 1 everywhere: a wrong batch stride of the blur or the resize mixes the values", (0, 1, 2), True))
    out.append(PyramidCase("constant-pow2-65x67", (2.0 ** torch.arange(3)).view(3, 1, 1, 1).expand(3, 1, 65, 67).contiguous(), SIZES[(65, 67)],
                           "image b is 2^b everywhere, odd sides", (0, 1), True))
    imp = torch.zeros(len(IMPULSES_64), 1, 64, 64)
    for b, (y, x) in enumerate(IMPULSES_64):
        imp[b, 0, y, x] = 63.0
    out.append(PyramidCase("impulses-64x64", imp, SIZES[(64, 64)],
                           "one pixel of 63 at each corner-side position: the reflect border without edge repeat, exactly", (0, 1)))
    g = torch.Generator().manual_seed(330)
    out.append(PyramidCase("integers-128x160", torch.randint(0, 64, (1, 1, 128, 160), generator=g).float(), SIZES[(128, 160)],
                           "integers 0..63: level 1 exact in fp32", (0, 1)))
    for H, W in ((65, 67), (97, 131)):
        out.append(PyramidCase(f"ramp-{H}x{W}", ramp(H, W), SIZES[(H, W)],
                               "3x + 5y: level 1 is the ramp at the resize's source positions away from the 2-pixel border", (0,), False, True))
    return out


def ramp_level1(H, W):
    """the closed form of level 1 of ramp(H, W) where no blur tap is reflected: 3 sx + 5 sy at the source position of each pixel, and
    the mask of the pixels whose four sources lie at least 2 pixels inside"""
    ho, wo = H // 2, W // 2
    sy = (H / ho) * (torch.arange(ho, dtype=torch.float64) + 0.5) - 0.5
    sx = (W / wo) * (torch.arange(wo, dtype=torch.float64) + 0.5) - 0.5
    val = 5.0 * sy[:, None] + 3.0 * sx[None, :]
    oky = (sy.floor() >= 2) & (sy.floor() + 1 <= H - 3)
    okx = (sx.floor() >= 2) & (sx.floor() + 1 <= W - 3)
    return val, oky[:, None] & okx[None, :]


# ---------------------------------------------------------------- extract
def extract_images() -> Dict[str, torch.Tensor]:
    """two-levels 96 x 128, pow2 64 x 128, three-levels 128 x 160, portrait 160 x 96, constant3 (B = 3, image b is b + 1, 128 x 160).
    The corner pixels of two-levels are multiples of 0.25, so that the sum of 1024 copies is exact in any order."""
    two = rand_image(1, 96, 128, 340)
    two[0, 0, 0, 0], two[0, 0, 0, -1], two[0, 0, -1, 0], two[0, 0, -1, -1] = 0.5, 0.25, 0.75, 1.0
    return {"two-levels": two, "pow2": rand_image(1, 64, 128, 343), "three-levels": rand_image(1, 128, 160, 341),
            "portrait": rand_image(1, 160, 96, 342),
            "constant3": torch.arange(1, 4, dtype=torch.float32).view(3, 1, 1, 1).expand(3, 1, 128, 160).contiguous()}


@dataclass
class ExtractCase:
    name: str
    image: str                                        # key of extract_images()
    lafs: torch.Tensor                                # [B, N, 2, 3] float32
    levels: List[int]                                 # the level of each LAF of image 0 (the same for every image)
    edge: str
    closed: Optional[Dict[bool, torch.Tensor]] = None  # upright -> the exact raw patches [B, N, 1, 32, 32], where the case claims them
    labels: List[str] = field(default_factory=list)
    normalised: bool = True                           # False: the patches are constant up to rounding, (x - mean) / (std + 1e-6) is noise


def _laf(a00, a01, a10, a11, cx, cy):
    return [[a00, a01, cx], [a10, a11, cy]]


def closed_crop(image2d, M, cx, cy):
    """the patch of the LAF [16 M | (cx, cy)], M a signed permutation, integer centre: patch pixel (i, j) is the image at
    x = M00 (j - 15.5) + M01 (i - 15.5) + cx - 0.5, y likewise with row 1, clamped to the image"""
    h, w = image2d.shape
    u = 2 * torch.arange(PS, dtype=torch.int64) - 31                   # 2 (k - 15.5)
    X2 = M[0][0] * u[None, :] + M[0][1] * u[:, None] + 2 * cx - 1
    Y2 = M[1][0] * u[None, :] + M[1][1] * u[:, None] + 2 * cy - 1
    assert bool((X2 % 2 == 0).all()) and bool((Y2 % 2 == 0).all())
    return image2d[(Y2 // 2).clamp(0, h - 1), (X2 // 2).clamp(0, w - 1)]


I2, R90, R180, R270 = ((1, 0), (0, 1)), ((0, 1), (-1, 0)), ((-1, 0), (0, -1)), ((0, -1), (1, 0))
MIRROR_X, MIRROR_SWAP = ((-1, 0), (0, 1)), ((0, 1), (1, 0))


def _crop_case(name, image_key, image, items, edge):
    """items: (label, M, cx, cy); every LAF is at scale 16, level 0"""
    lafs = torch.tensor([[_laf(16.0 * M[0][0], 16.0 * M[0][1], 16.0 * M[1][0], 16.0 * M[1][1], float(cx), float(cy)) for _, M, cx, cy in items]])
    closed = {False: torch.stack([closed_crop(image[0, 0], M, cx, cy) for _, M, cx, cy in items])[None, :, None],
              True: torch.stack([closed_crop(image[0, 0], I2, cx, cy) for _, M, cx, cy in items])[None, :, None]}
    return ExtractCase(name, image_key, lafs, [0] * len(items), edge, closed, [i[0] for i in items])


def boundary_lafs(cx=70.0, cy=60.0):
    """scales 16, 32, 64, 128 and one fp32 step below each, axis-aligned and rotated by 90 degrees -> lafs [1, 16, 2, 3], levels"""
    rows, levels = [], []
    for k, s in enumerate((16.0, 32.0, 64.0, 128.0)):
        below = float(torch.nextafter(torch.tensor(s), torch.tensor(0.0)))
        for v, lev in ((s, k), (below, max(k - 1, 0))):
            rows += [_laf(v, 0.0, 0.0, v, cx, cy), _laf(0.0, v, -v, 0.0, cx, cy)]
            levels += [lev, lev]
    return torch.tensor([rows]), levels


def extract_cases():
    im = extract_images()
    out = []
    two, H, W = im["two-levels"], 96, 128
    out.append(_crop_case("crops", "two-levels", two, [
        ("identity", I2, 40, 50), ("rot90", R90, 40, 50), ("rot180", R180, 40, 50), ("rot270", R270, 40, 50),
        ("mirror-x", MIRROR_X, 40, 50), ("mirror-swap", MIRROR_SWAP, 40, 50),
        ("clamp-left", I2, 5, 50), ("clamp-right", I2, W - 5, 50), ("clamp-bottom", I2, 40, H - 5),
        ("outside-top-left", I2, -40, -40), ("outside-bottom-right", R180, W + 60, H + 50),
        ("far-right", I2, 10000, 50), ("far-left", R90, -10000, 50), ("far-above", I2, 40, -10000), ("far-corner", I2, 10000, 10000)],
        "scale 16, integer centre: every sample is a pixel; rotations, mirrors (det < 0), the clamp on each border, patches outside"))
    out.append(_crop_case("crops-portrait", "portrait", im["portrait"], [
        ("identity", I2, 40, 90), ("rot90", R90, 40, 90), ("mirror-x", MIRROR_X, 50, 100), ("clamp-corner", I2, 92, 155)],
        "h > w: the level ratio takes min(h, w) = w, which is not h"))
    out.append(_crop_case("crops-pow2", "pow2", im["pow2"], [
        ("clamp-top", I2, 40, 5), ("clamp-bottom", R180, 40, 59), ("clamp-left", R90, 5, 30), ("clamp-right", R270, 123, 30),
        ("corner-top-left", R90, 3, 4), ("corner-top-right", I2, 125, 2), ("corner-bottom-left", MIRROR_X, 6, 60),
        ("corner-bottom-right", MIRROR_SWAP, 120, 58), ("covers-the-height", I2, 64, 32)],
        "64 x 128, both sides powers of two, where the restatement's grid round trip is exact at the top rows as well: every border, every corner"))
    top = torch.tensor([[_laf(16.0, 0.0, 0.0, 16.0, 40.0, 5.0), _laf(0.0, 16.0, -16.0, 0.0, 3.0, 4.0)]])
    out.append(ExtractCase("clamp-top-96", "two-levels", top, [0, 0],
                           "the top border at height 96, where the restatement itself is 3e-15 from the crop: held to the rule", None))
    lafs, levels = boundary_lafs()
    out.append(ExtractCase("boundaries-three-levels", "three-levels", lafs, levels,
                           "scale 16 * 2^k exactly and one fp32 step below, k = 0..3; level 2 is built, level 3 is not"))
    out.append(ExtractCase("boundaries-two-levels", "two-levels", lafs.clone(), levels,
                           "the same LAFs where level 2 is not built: exact zeros, raw and normalised"))
    mir = torch.tensor([[_laf(-32.0, 0.0, 0.0, 32.0, 70.0, 60.0), _laf(0.0, 40.0, 40.0, 0.0, 64.3, 50.7), _laf(-20.0, 3.0, 5.0, 90.0, 60.0, 64.0)]])
    out.append(ExtractCase("mirrored-level-1", "three-levels", mir, [1, 1, 1], "det < 0 at scales 32, 40, 42.6: |det| decides the level"))
    deg = torch.tensor([[_laf(0.0, 0.0, 0.0, 0.0, 40.5, 50.5), _laf(0.0, 0.0, 0.0, 0.0, 40.25, 50.75), _laf(8.0, 4.0, 4.0, 2.0, 60.5, 30.5),
                         _laf(1e6, 0.0, 0.0, 1e6, 60.0, 40.0), _laf(0.0, 1e6, -1e6, 0.0, 60.0, 40.0)]])
    out.append(ExtractCase("degenerate", "two-levels", deg, [0, 0, 0, 15, 15],
                           "A = 0 (a constant patch: the bilinear value at the centre), a singular A, scale 1e6 (level >= 12: zeros)"))
    c3 = torch.tensor([_laf(16.0, 0.0, 0.0, 16.0, 70.0, 60.0), _laf(0.0, 16.0, -16.0, 0.0, 3.0, 120.0), _laf(32.0, 0.0, 0.0, 32.0, 70.0, 60.0),
                       _laf(30.0, 25.0, -25.0, 30.0, 100.3, 40.6), _laf(64.0, 0.0, 0.0, 64.0, 80.0, 64.0)])
    out.append(ExtractCase("constant3", "constant3", c3[None].repeat(3, 1, 1, 1), [0, 0, 1, 1, 2],
                           "B = 3, image b is b + 1: a wrong batch stride at level 0, 1 or 2 reads another image's value", normalised=False))
    return out


def kernel_level(lafs):
    """the level decision of pn_extract_kernel restated in float32: sc = sqrt |det| with the determinant rounded once, then
    t = sc / 16 halved while t >= 2, at most 12 times"""
    A = lafs.float()
    det = (A[..., 0, 0].double() * A[..., 1, 1].double() - A[..., 0, 1].double() * A[..., 1, 0].double()).float()   # exact here: one product is 0
    t = det.abs().sqrt() * torch.tensor(1.0 / 16.0)
    lev = torch.zeros_like(t, dtype=torch.int64)
    for _ in range(12):
        go = t >= 2.0
        lev = lev + go.long()
        t = torch.where(go, t * 0.5, t)
    return lev


# ---------------------------------------------------------------- networks
def random_patches(n, seed):
    """n patches of different content, scale and mean"""
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, 1, PS, PS, generator=g) * (0.5 + torch.rand(n, 1, 1, 1, generator=g)) + torch.randn(n, 1, 1, 1, generator=g)


def random_lafs(n, seed):
    """n different LAFs: entries ~ 8 N(0, 1), centres in [0, 90)"""
    g = torch.Generator().manual_seed(seed)
    lafs = torch.randn(n, 2, 3, generator=g) * 8
    lafs[:, :, 2] = torch.rand(n, 2, generator=g) * 90
    return lafs


SEAM_N = (512, 513, 515)     # one full chunk; a second pass of 1 (a lone patch in an 8 x 8 pair); a second pass of 3
SMALL_N = (1, 31, 32, 33)    # the HardNet tail's 32-row tile: one short, full, one over
SEAM_UNIQUE = 7              # coprime to 512: patch 512 + i is not patch i


def seam_index(n):
    return torch.arange(n) % SEAM_UNIQUE


def _state_dict(kind, seed=2):
    from openglue_amd import synthetic as syn
    return syn.make_patchnet_state_dict(kind, seed=seed)


def dead_patches():
    """four random patches, a zero patch and a bright diagonal"""
    return torch.cat([random_patches(4, 60), torch.zeros(1, 1, PS, PS), 63.0 * torch.eye(PS)[None, None]])


def dead_trunk(kind, tail_mean_zero=True, bias=None, seed=2):
    """a state dict whose hidden BatchNorms all have a positive running mean (1000 behind features.0, |mean| + 0.01 behind the
    others): every ReLU output is 0, so the 8 x 8 convolution sees zeros"""
    sd = _state_dict(kind, seed)
    for i in (0, 3, 6, 9, 12, 15):
        k = f"features.{i + 1}.running_mean"
        sd[k] = torch.full_like(sd[k], 1000.0) if i == 0 else sd[k].abs() + 0.01
    if kind == "hardnet":
        if tail_mean_zero:
            sd["features.20.running_mean"] = torch.zeros(128)
    elif bias is not None:
        sd["features.19.bias"] = torch.tensor(bias, dtype=torch.float32)
    return sd


def chosen_tanh(kind, target=None, bias=None, seed=2):
    """a state dict with a zero tail weight and bias = atanh(target) (or the bias itself): every patch gives tanh(bias)"""
    sd = _state_dict(kind, seed)
    sd["features.19.weight"] = torch.zeros_like(sd["features.19.weight"])
    b = torch.tensor(bias, dtype=torch.float64) if bias is not None else torch.atanh(torch.tensor(target, dtype=torch.float64))
    sd["features.19.bias"] = b.float()
    return sd


Q = 0.5
ORINET_TARGETS = {"quadrant-1": (Q, Q), "quadrant-2": (Q, -Q), "quadrant-3": (-Q, -Q), "quadrant-4": (-Q, Q),
                  "axis+y1": (0.0, 0.7), "axis-y1": (0.0, -0.7), "axis+y0": (0.7, 0.0), "axis-y0": (-0.7, 0.0),
                  "zero-45-degrees": (0.0, 0.0), "hypot-zero": (-1e-8, -1e-8)}
AFFNET_TARGETS = {"zero": (0.0, 0.0, 0.0), "+0.9": (0.9, 0.9, 0.9), "-0.9": (-0.9, -0.9, -0.9), "mixed-0.9": (0.9, -0.9, -0.9)}
AFFNET_BIASES = {"bias+4": (4.0, 4.0, 4.0), "bias-4": (-4.0, -4.0, -4.0), "bias-4+4-4": (-4.0, 4.0, -4.0), "bias+4-4-4": (4.0, -4.0, -4.0)}

# the LAFs every chosen output is applied to: a00 = a01 = 0 (hypot 0 in AffNet's orientation), det < 0, a similarity, anisotropic
UPDATE_LAFS = torch.tensor([_laf(0.0, 0.0, 5.0, 7.0, 11.0, 12.0), _laf(0.0, 0.0, -3.0, 0.0, 13.0, 14.0), _laf(9.0, 2.0, 3.0, -4.0, 15.0, 16.0),
                            _laf(6.0, 8.0, -8.0, 6.0, 17.0, 18.0), _laf(12.0, -3.0, 1.5, 4.0, 19.0, 20.0), _laf(-7.0, 0.0, 0.0, 7.0, 21.0, 22.0)])
UPDATE_LABELS = ["a00=a01=0", "a00=a01=0, det=0", "det<0", "similarity", "anisotropic", "ori=180"]
