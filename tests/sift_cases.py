"""Crafted inputs for the stage-level tests of the SIFT extractor (csrc/sift.hip: sift_extrema_kernel / sift_refine / sift_compact_kernel,
sift_orient_kernel / sift_expand_kernel, sift_describe_kernel, the selection kernels).  tests/test_sift_cases_cpu.py proves on the CPU,
with the float64 restatement (tests/sift_ref.py), that every case reaches the edge it names; tests/test_gpu_sift_stages.py feeds the
same arrays to the stage methods of openglue_amd.sift.SIFT and holds the kernels to the restatement.

NumPy only and deterministic.  The DoG volumes hold integers as fp32 (so every comparison of the extremum test and every fp64 product
of the refinement is exact on both sides) except the `big` stencil, whose integers are below 2^23 and whose fp64 products round the
same way on both sides because both use the same operation order.  Random blocks were found by a seeded search on the CPU
(numpy.random.default_rng(0), 5 x 8 x 8 integers in [-40, 40] at rows and columns 12 .. 19 of a 32 x 32 octave) and are frozen here
as literal arrays.

Image sizes are the smallest that reach the edge: 8 x 8 builds one octave of 16 x 16 (cap 1024, cap2 1280, 40960 neighbour entries),
16 x 16 two octaves (32 x 32 and 16 x 16), 24 x 40 three, 8 x 136 one octave of 16 x 272 (two 256-column segments per row).
"""
from dataclasses import dataclass, field
from typing import List, Optional, Tuple

import numpy as np

import sift_ref as R

SEG = 256                    # SIFT_SEG of the source: columns per detection segment
MAX_PEAKS = 18               # SIFT_MAX_PEAKS
NBR_AVG = 32                 # SIFT_NBR_AVG


def capacities(H, W):
    """(cap, cap2, capn) of sift_geom: keypoints, oriented keypoints and NMS neighbour entries per image"""
    cap = max(4 * H * W // 8, 1024)
    cap2 = cap + cap // 4
    return cap, cap2, NBR_AVG * cap2


def zero_dog(H, W):
    return [np.zeros((R.S + 2, h, w), dtype=np.float32) for h, w in R.octave_sizes(H, W)]


def zero_gauss(H, W):
    return [np.zeros((R.S + 3, h, w), dtype=np.float32) for h, w in R.octave_sizes(H, W)]


# ---------------------------------------------------------------- detect
@dataclass
class DetectCase:
    name: str
    H: int
    W: int
    dog: List[List[np.ndarray]]                       # [image][octave] float32 [5, h, w]
    edge: str
    claims: List[Tuple[int, Tuple[int, int, int, int], str, Optional[int]]] = field(default_factory=list)
    #        (image, (octave, layer, row, column) of a candidate, its exit in R.EXITS, the steps it takes or None)
    kept: Optional[List[int]] = None                  # keypoints per image, where the case says so
    candidates: Optional[List[int]] = None            # candidates per image, likewise
    stage: str = "detect"


def stencil(A, cf=None, rf=None, lf=None, rc=None, lc=None, lr=None, fill=None):
    """3 x 3 x 3 samples [dl + 1][dr + 1][dc + 1] around a centre of value A: faces (minus, plus) along column, row and layer,
    in-plane and cross-layer edge quadruples (pp, pm, mp, mm) as the mixed differences read them, everything else `fill`"""
    fill = A - 10 if fill is None else fill
    s = np.full((3, 3, 3), float(fill))
    s[1, 1, 1] = A
    for ax, f in ((2, cf), (1, rf), (0, lf)):
        m, p = (fill, fill) if f is None else f
        i = [1, 1, 1]
        i[ax] = 0
        s[tuple(i)] = m
        i[ax] = 2
        s[tuple(i)] = p
    for (a, b), q in (((1, 2), rc), ((0, 2), lc), ((0, 1), lr)):
        if q is None:
            continue
        for (sa, sb), v in zip(((2, 2), (2, 0), (0, 2), (0, 0)), q):
            i = [1, 1, 1]
            i[a], i[b] = sa, sb
            s[tuple(i)] = v
    return s


def put(d, l, r, c, s):
    """stencil s, whose centre is its sample [1, 1, 1], on sample (l, r, c) of the octave volume d"""
    nl, nr, nc = s.shape
    d[l - 1:l - 1 + nl, r - 1:r - 1 + nr, c - 1:c - 1 + nc] = s


def bump(A=20.0, sign=1.0):
    """A - dc^2 - dr^2 - dl^2: converges at once with offset 0"""
    g = np.arange(-1, 2, dtype=np.float64) ** 2
    return sign * (A - g[None, None, :] - g[None, :, None] - g[:, None, None])


def bump_offset():
    """16 * 20 - (4 dc - 1)^2 - (4 dr - 1)^2 - (4 dl - 1)^2: the maximum of the quadratic lies at +0.25 on every axis"""
    g = (4.0 * np.arange(-1, 2, dtype=np.float64) - 1.0) ** 2
    return 320.0 - g[None, None, :] - g[None, :, None] - g[:, None, None]


def tie_pair(A=20.0):
    """3 x 3 x 4: two equal maxima side by side.  The left one sees an offset of exactly +0.5 and steps onto the right one, which
    sees exactly -0.5, rounds it half up to 0 and stays: five steps, nothing kept"""
    gc = np.array([2.0, 0.0, 0.0, 2.0])
    g = np.arange(-1, 2, dtype=np.float64) ** 2
    return A - gc[None, None, :] - g[None, :, None] - g[:, None, None]


def mover(axis, sign, A=50.0):
    """a maximum whose quadratic has dxx = dyy = dss = -20, one mixed derivative of 19 and a gradient of 5: offsets of 2.56 and 2.44
    (-2, 1.9 and 0.5 times ten, to stay in integers).  axis "c" / "r": the pair is (column, row) and the larger step of 3 goes along
    `axis`, the step of 2 along the other; axis "l": the pair is (layer, column), 3 layers and 2 columns.  sign: the direction."""
    lo, hi = (A - 15, A - 5) if sign > 0 else (A - 5, A - 15)
    same = (A - 10, A - 10)
    cross = (A - 2, A - 40, A - 40, A - 2)
    if axis == "c":
        return stencil(A, cf=(lo, hi), rf=same, lf=same, rc=cross)
    if axis == "r":
        return stencil(A, cf=same, rf=(lo, hi), lf=same, rc=cross)
    return stencil(A, cf=same, rf=same, lf=(lo, hi), lc=cross)


def big_stencil():
    """near-singular in the (column, row) plane: dxx = dyy = -2^21, dxy = 2^21 - 1/4, gx = 2^20, so both in-plane offsets are about
    2^21 >= 1e6.  Integers below 2^23, exact in fp32"""
    N = float(2 ** 20)
    A = 2 * N
    return stencil(A, cf=(A - 2 * N, A), rf=(A - N, A - N), lf=(A - 1, A - 1), rc=(A, A - 4 * N, A - 4 * N + 1, A), fill=A - 1)


def _blk(rows):
    return np.array(rows, dtype=np.float32).reshape(5, 8, 8)


# draw 8: candidate (2, 13, 19) moves a layer down and a row on and converges on (1, 14, 19); (3, 13, 14) moves a column back
MIXED = _blk([[35, 14, 14, 17, 22, -24, 39, 35, 18, -14, -38, 7, 26, -32, 21, 40, -28, 12, 1, -3, 36, 5, -34, -38, -18, -21, 24, 38, -2, -34, 19, -29, 24, 6, -12, 22, -36, 29, -24, 29, -4, 21, -22, -12, 40, 7, -14, 25, -1, -29, 34, -34, 7, -3, 7, -15, -14, -40, 38, 1, 30, -10, 34, 31], [-1, -13, -33, 13, 0, 6, -21, -16, 5, -3, 10, -11, 10, -21, -11, -33, 24, -36, -37, -22, 16, -34, 37, -28, 25, -30, -21, -10, 28, -21, 14, -40, -21, -38, -21, 40, 10, -21, 21, -37, -24, 10, 14, 4, -38, -9, 20, 19, -33, 35, 11, -8, 36, -10, -13, 1, -40, -22, -7, -26, 24, -9, 4, 14], [-33, -39, 15, -29, 34, 25, -31, -14, 38, 5, -21, -36, -33, 4, 27, -38, -12, -24, 17, -4, -25, 2, 24, -30, -31, -3, -28, 23, 11, 17, -6, -11, -21, 0, 7, 24, 29, -19, 32, -29, 7, 38, 7, 30, -7, 30, 13, -2, 9, -38, -28, 20, 29, 24, -4, 38, -17, -38, -25, 25, -34, -13, -4, 13], [11, 32, 15, -20, -38, 40, 25, -37, -37, -31, -39, -2, -1, 18, -26, 35, -35, 28, -3, 38, -29, -5, 4, -8, -38, 7, 21, 16, 12, 33, -29, 7, 15, 33, 38, -7, -39, 22, 30, 40, 18, -34, 38, 17, 37, 33, 19, 32, 2, 30, 24, -18, 7, -8, -18, 1, 29, 38, -24, -19, -20, 13, 19, 21], [21, -29, -13, 30, -37, 0, 26, 37, -30, 32, -31, 36, -27, -26, -17, 27, 1, 29, -38, 36, 18, 12, -12, -11, -6, 7, 21, -28, 28, 40, 14, 18, 26, -13, -12, 34, -31, 17, 25, -14, -12, 35, -25, -14, 17, -15, 18, -38, -11, 16, 34, -32, 3, -37, -25, 13, 1, 38, 26, -35, 28, 21, -22, -22]])
# draw 35: candidate (2, 15, 19) moves up onto layer 3, the last one, and converges there
LAYER3 = _blk([[-21, 5, -37, -28, 37, 5, -7, -15, -18, 38, 34, -34, 5, 31, 15, -11, 24, -37, -38, 28, -30, -32, 13, -39, -10, 7, 25, 19, -32, 27, 15, -16, 40, -6, -21, 9, -38, -11, 10, 36, -9, 6, 7, -15, -34, 14, 25, 18, 4, 39, -21, -9, -8, 29, -20, 7, 38, 0, -13, 7, -2, 35, -4, 21], [-31, 34, 18, 13, -30, 34, -6, -32, 29, -34, 14, -3, -19, -21, 32, -13, 38, -8, 12, -24, 34, 29, -25, 3, 1, -8, 0, 0, 0, -40, 8, -23, -13, 36, 1, -22, 17, -38, -6, 14, 11, 26, 0, -6, 24, 16, 25, 19, 40, -18, 15, 17, 0, -37, 33, 26, 17, 13, -39, -25, -28, -14, -38, -38], [24, -39, 39, -6, 32, 32, -22, -6, -18, 0, 36, 12, 3, 7, -22, -33, -29, 7, 6, -17, -5, -38, -32, -38, -4, -10, 40, 27, -12, -38, -25, 39, 22, -15, -16, -22, -5, 2, 4, -34, -27, -29, 13, 18, -37, 8, -37, -8, -34, 7, 38, -15, -26, 8, 6, 6, -5, 13, 35, -36, -15, 16, 21, 1], [32, 35, 21, 28, 32, -1, -17, 11, -24, -3, -31, 9, 12, -16, 30, 0, -33, -38, -11, 5, 33, -2, 11, -21, -39, 27, 31, 26, -20, -1, -6, 39, 19, -3, -18, -1, -39, 16, -13, 13, -15, -15, 4, 36, -36, 33, 19, -35, -38, -28, 6, 15, 10, 0, -15, -29, -1, -9, 2, -8, -7, 6, -32, 22], [8, -11, -27, 14, -11, 13, -26, 3, 33, 8, 10, -28, -22, -2, 7, -6, 38, 5, -40, 2, -31, -40, -5, 1, 23, -1, -40, -20, 33, -5, -25, -33, 16, 30, 21, 31, -13, 34, -26, 23, 23, 30, -14, 11, -28, 19, -32, -3, 34, 11, 40, -35, 24, 6, -5, -13, -12, -34, 40, -5, -40, 24, 21, 28]])
# draw 42: candidate (1, 18, 14) moves one column on and converges on (1, 18, 15)
CPLUS = _blk([[33, -34, -7, -27, 27, -33, 21, -12, 0, 21, 13, -24, -6, 26, 3, -25, -25, 2, 34, -27, 33, -5, 23, -37, 2, -23, -36, 40, -33, 5, -11, 32, -3, -10, 39, -12, -25, -17, -33, -37, 34, 0, 39, 17, 22, 8, 15, -5, 12, -25, -8, 19, 28, 16, 34, -7, 20, -27, 13, 24, 16, 33, -15, 12], [-22, -2, -39, 32, -6, -16, 23, -1, -8, 40, 23, -25, -38, 15, 6, -3, -13, 22, -24, 40, 27, 7, 3, 19, 13, -10, -33, -20, -38, 10, 34, -25, -37, 16, -3, -4, -12, -37, 35, -16, -22, 34, -21, 33, 31, 7, -28, -10, -33, 15, -39, -38, -38, 17, -23, 3, -22, 18, -2, 40, 14, 15, -24, 33], [-26, -8, -39, 36, 22, 40, 22, 32, 22, -34, 7, -34, -5, 28, -36, 24, 32, -36, 3, -35, -25, 25, 13, -15, 28, -11, 19, -9, -5, -39, 16, 4, 10, -31, 33, 12, 1, -33, -23, 37, 5, 28, -24, 19, 4, -38, 19, -2, 21, -22, -11, -10, -9, 5, 32, 18, 13, 7, -2, -27, 22, -26, -10, 6], [-19, -19, -38, 10, 19, -26, -35, 28, -17, 0, -21, 3, 20, 18, -33, 9, 1, 27, -10, -24, -25, 25, -38, 23, 20, -24, -11, -36, -11, -30, -33, -4, 7, 4, -15, -22, 40, -2, 33, -6, -4, 12, -30, 25, -10, -31, -12, 40, 37, -15, 29, -35, 31, 4, -32, -27, 38, 21, 36, -31, 13, -21, -14, 21], [37, 35, -21, -9, -9, 23, 13, 16, 35, 8, -6, 2, 33, -35, 4, 16, 7, 33, -2, -26, 2, -10, -15, -18, 35, -17, -11, 11, 20, -22, -9, 2, -31, 36, -39, -29, -17, 16, -20, -25, -22, -22, -35, -36, -16, 23, -5, -37, 35, -5, 4, 8, -21, 20, 39, -11, 3, 25, -20, -31, 40, -14, 0, -35]])
# draw 3: candidates (3, 12, 14) and (2, 13, 14) both end on (1, 13, 14), in the fourth and in the fifth, the last, step
STEP5 = _blk([[18, -11, 40, 6, 13, 2, 24, -12, 9, 11, 30, 14, 8, 5, -36, -9, -15, 10, -15, 7, 0, -13, 1, -16, -23, 4, 40, 9, 9, 9, 31, -9, -6, 5, 5, 39, -26, -6, -23, 28, 4, -34, -26, 30, -5, 36, -33, -19, 4, -40, -9, -1, -21, -26, 35, 38, 0, 32, -1, 37, -37, 8, -37, 1], [31, 27, -23, 12, -27, -20, -6, 35, 14, -5, -24, 22, 7, 0, 12, -26, 34, -17, -2, 6, -26, -29, -2, -39, 8, -5, -21, 21, -14, 9, -24, -14, 10, 18, 11, -1, -20, 40, 33, 22, -17, 27, 6, -19, 23, -28, 6, -24, -35, -5, -4, 1, -40, -25, -34, 23, -36, 30, -23, -15, -13, 1, -11, 8], [-10, 18, 40, -29, -31, -18, -24, 19, 18, 6, 40, 32, 39, -4, 4, -8, -18, -16, 20, -22, -29, 12, 3, -19, -16, 29, -37, -19, 5, 14, 6, 6, 22, 10, 10, 32, 21, -27, 38, -28, 36, -31, 39, -34, 31, 3, 5, -27, -30, 25, -21, -39, -4, -10, -4, -2, -35, -23, -19, -12, -6, -22, 24, -18], [-5, 35, 40, -7, -9, -9, -12, 9, 11, 13, 23, 13, -19, -34, -7, 7, 34, 19, -15, 24, 13, 7, 29, -30, -1, -34, 20, -14, 22, 35, 29, -2, 10, 32, -31, -3, -17, 21, 40, -1, -4, 17, -20, -15, -27, 32, 1, -19, 10, -40, -11, 18, 38, 14, -30, 13, 17, 15, -29, 7, -9, -31, 39, 14], [28, -40, -7, -26, 33, -6, 13, -10, 35, -31, -30, -6, 7, 10, 30, -10, 36, 17, 6, -22, 20, -29, -36, 20, -21, 14, 5, -6, -4, -29, -16, 13, -10, 20, 36, -27, -25, 15, -20, -12, 33, 34, 34, 20, -37, -18, 11, 35, -20, -38, 16, -26, 31, -21, -30, 19, -24, 2, 38, -3, -17, -22, 0, 21]])
# draw 215: candidate (1, 14, 14) uses up its five steps and would converge on (1, 19, 15) in a sixth
SIX = _blk([[6, 25, 19, 6, 24, 24, 35, 8, -13, 15, -23, 4, 8, 24, 0, 8, 27, 37, 29, 23, 6, 20, 19, -2, 16, -9, -26, 27, -32, -15, 36, -7, 6, 4, 29, 9, -23, -14, -38, -33, -10, -17, 2, 16, 9, 36, 0, 13, -23, -21, -18, -17, -30, -11, -8, 23, 18, 27, 14, 15, -14, 28, -34, -30], [27, -28, 1, 15, 10, 13, -31, -19, -36, 20, 22, 9, 24, -29, 9, -5, -26, -32, -34, 30, 37, -7, 38, 24, -39, -10, -32, 29, -3, 6, 39, 22, 30, 3, -27, -35, -29, -4, 4, 5, -26, 32, -18, 35, 8, -28, 6, -15, -28, -12, 6, -10, -28, -13, 28, 10, 26, 3, -20, -40, -10, -12, -35, 40], [-28, 14, 26, 3, -10, -23, -5, -4, -23, -21, 31, 13, 7, 32, -4, -19, 10, -9, -32, 7, 30, 20, 7, 29, 30, -9, -30, -5, 22, -21, 30, -38, 27, 40, -9, -40, -20, 9, -37, -34, -37, -23, -9, -39, -40, 24, -17, 18, 23, -30, -10, -12, 2, 36, -28, 27, 3, -29, -35, 5, -7, -20, 17, -28], [7, 9, 25, -19, -24, -33, 13, -40, 27, 31, -18, -34, -35, 6, -10, 39, -34, -38, -21, 17, 19, -31, 9, -10, -31, 39, 26, 0, -25, 28, -13, 14, -16, 16, 2, 24, 24, -6, -28, 29, 17, 39, -11, -23, -2, -32, -6, -2, -22, 7, -35, -36, -13, -31, 29, 17, -37, 37, -34, 32, 18, -25, -31, -16], [16, -6, 15, -5, 6, -28, 5, -34, -32, 9, 28, 17, 8, 22, 1, -12, 10, 38, 7, -9, -13, -32, 32, 35, 8, -26, -22, 21, 11, 2, 6, 8, -18, 9, -28, -34, 17, 16, 36, 39, -39, -27, 24, 40, -31, 29, 34, 25, -20, -35, 31, -8, -23, -20, 28, -19, 26, -37, 22, -12, -11, -6, -13, 28]])


def block_volume(blk, r0=12, c0=12):
    """a found block in octave 0 of a 16 x 16 image (32 x 32; octave 1 stays zero)"""
    dog = zero_dog(16, 16)
    dog[0][:, r0:r0 + 8, c0:c0 + 8] = blk
    return dog


def checkerboard(H, W):
    """d[l, r, c] = s[l] * (+1 if (r + c) even else -1), s = 8, 16, 8, 16, 8, in every octave: every interior sample of layers 1
    and 3 is an extremum that converges at once with response 16 / 255"""
    out = []
    for h, w in R.octave_sizes(H, W):
        rr, cc = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
        sign = np.where((rr + cc) % 2 == 0, 1.0, -1.0)
        out.append((np.array([8.0, 16.0, 8.0, 16.0, 8.0])[:, None, None] * sign[None]).astype(np.float32))
    return out


def checkerboard_count(H, W):
    return sum(2 * (h - 2 * R.BORDER) * (w - 2 * R.BORDER) for h, w in R.octave_sizes(H, W))


def sparse_dog(H, W):
    """a few bumps, one per octave and a minimum: the quiet neighbour of an overflowing image"""
    dog = zero_dog(H, W)
    for o, d in enumerate(dog):
        _, h, w = d.shape
        put(d, 1 + o % 3, R.BORDER, w - R.BORDER - 1, bump(20.0 + o))
        put(d, 3 - o % 3, h - R.BORDER - 1, R.BORDER, bump(30.0 + o, -1.0))
    return dog


def detect_cases():
    out = []

    def add(*a, **k):
        out.append(DetectCase(*a, **k))

    # converged at once
    d = zero_dog(8, 8)
    put(d[0], 2, 6, 6, bump())
    put(d[0], 2, 6, 10, bump_offset())
    put(d[0], 2, 10, 6, bump(20.0, -1.0))
    add("bumps", 8, 8, [d], "converged at once: offset 0, offset 0.25 on every axis, a minimum",
        claims=[(0, (0, 2, 6, 6), "converged", 1), (0, (0, 2, 6, 10), "converged", 1), (0, (0, 2, 10, 6), "converged", 1)],
        kept=[3], candidates=[3])
    # tie pair
    d = zero_dog(8, 8)
    put(d[0], 2, 8, 7, tie_pair())
    add("tie-pair", 8, 8, [d], "two adjacent equal maxima are both candidates under >=, see offsets of exactly +-0.5 and use up "
        "five steps", claims=[(0, (0, 2, 8, 7), "steps", 5), (0, (0, 2, 8, 8), "steps", 5)], kept=[0], candidates=[2])
    # plateau and zero
    d = zero_dog(8, 8)
    d[0][:] = 7.0
    add("plateau", 8, 8, [d], "a constant non-zero volume: every interior sample is a candidate with det == 0",
        claims=[(0, (0, l, r, c), "det0", 1) for l in (1, 3) for r, c in ((5, 5), (10, 10), (7, 8))], kept=[0], candidates=[3 * 36])
    add("zero", 8, 8, [zero_dog(8, 8)], "the same volume at 0: the v != 0 skip leaves no candidate", kept=[0], candidates=[0])
    d = zero_dog(8, 8)
    put(d[0], 2, 7, 7, bump(0.0, -1.0))
    put(d[0], 2, 10, 10, -bump(0.0, -1.0))
    add("zero-extrema", 8, 8, [d, sparse_dog(8, 8)], "a sample of value 0 below 26 positive neighbours, and one above 26 negative ones: "
        "extrema in everything but the sign test, which the v != 0 skip stands for; without it they converge at once with response 0.  (The corners of the two blocks are "
        "extrema against the zero background and are kept.)", kept=[10, 2], candidates=[10, 2])
    d = zero_dog(8, 8)
    d[0][:] = -7.0
    add("plateau-negative", 8, 8, [d], "a constant negative volume: every interior sample is a candidate (<= its neighbours)",
        kept=[0], candidates=[3 * 36])
    # long moves out of the border and out of the layers (octave 0 of 16 x 16: 32 x 32)
    d = zero_dog(16, 16)
    w = 32
    put(d[0], 2, 8, w - 6, mover("c", +1))
    put(d[0], 2, 16, 5, mover("c", -1))
    put(d[0], 2, w - 6, 12, mover("r", +1))
    put(d[0], 2, 5, 20, mover("r", -1))
    put(d[0], 2, 16, 16, mover("l", +1))
    put(d[0], 2, 22, 22, mover("l", -1))
    put(d[0], 2, 12, w - 8, mover("c", +1))              # lands on column w - 5 exactly
    put(d[0], 2, 22, 7, mover("c", -1))                  # lands on column 4 exactly
    add("long-moves", 16, 16, [d], "offsets of 2.56 and 2.44: out of the border in all four directions, out of layers 1 .. 3 upwards and "
        "downwards, onto the first column outside the border on either side",
        claims=[(0, (0, 2, 8, w - 6), "border", 1), (0, (0, 2, 16, 5), "border", 1), (0, (0, 2, w - 6, 12), "border", 1),
                (0, (0, 2, 5, 20), "border", 1), (0, (0, 2, 16, 16), "layer", 1), (0, (0, 2, 22, 22), "layer", 1),
                (0, (0, 2, 12, w - 8), "border", 1), (0, (0, 2, 22, 7), "border", 1)], kept=[0], candidates=[8])
    # moved, then converged: the found blocks
    add("moved-mixed", 16, 16, [block_volume(MIXED)], "moved within the plane, and across a layer, then converged",
        claims=[(0, (0, 3, 13, 14), "converged", 2), (0, (0, 2, 13, 19), "converged", 2)])
    add("moved-to-layer3", 16, 16, [block_volume(LAYER3)], "moved up onto layer 3, the last one allowed, and converged there",
        claims=[(0, (0, 2, 15, 19), "converged", 2)])
    add("moved-one-column", 16, 16, [block_volume(CPLUS)], "moved one column on and converged",
        claims=[(0, (0, 1, 18, 14), "converged", 2)])
    add("moved-onto-border", 16, 16, [block_volume(CPLUS, 12, 24)], "the same block 12 columns further right: the move from column "
        "w - 6 lands on w - 5, the first column outside, where the sample would have converged",
        claims=[(0, (0, 1, 18, 26), "border", 1)])
    add("fifth-step", 16, 16, [block_volume(STEP5)], "converged in the fourth and in the fifth, the last, step",
        claims=[(0, (0, 3, 12, 14), "converged", 4), (0, (0, 2, 13, 14), "converged", 5)])
    add("sixth-step", 16, 16, [block_volume(SIX)], "five steps used up where a sixth would have converged",
        claims=[(0, (0, 1, 14, 14), "steps", 5)])
    # offsets >= 1e6
    d = zero_dog(8, 8)
    put(d[0], 2, 8, 7, big_stencil())
    add("big", 8, 8, [d], "a near-singular Hessian: offsets of about 2^21, over the 1e6 line",
        claims=[(0, (0, 2, 8, 7), "big", 1)])
    # geometry: segment seams, first and last interior row and column, first and last layer, two different images
    H, W = 8, 136
    a, b = zero_dog(H, W), zero_dog(H, W)
    h, w = a[0].shape[1:]
    sites_a = [(1, 5, 5), (3, h - 6, w - 6), (1, 5, SEG - 1), (3, h - 6, SEG + 1), (3, 5, 100)]
    sites_b = [(2, 7, SEG), (1, h - 6, 5), (3, 5, w - 6), (1, h - 6, 200)]
    for i, (l, r, c) in enumerate(sites_a):
        put(a[0], l, r, c, bump(20.0 + i))
    for i, (l, r, c) in enumerate(sites_b):
        put(b[0], l, r, c, bump(40.0 + i, -1.0 if i % 2 else 1.0))
    add("geometry-seam", H, W, [a, b], "columns 5, w - 6, 255, 256, 257 of a 272-wide octave (two segments per row), rows 5 and "
        "h - 6, layers 1 and 3, two images with different volumes",
        claims=[(0, (0,) + s, "converged", 1) for s in sites_a] + [(1, (0,) + s, "converged", 1) for s in sites_b],
        kept=[len(sites_a), len(sites_b)], candidates=[len(sites_a), len(sites_b)])
    H, W = 24, 40
    a, b = zero_dog(H, W), sparse_dog(H, W)
    claims = []
    for o, d in enumerate(a):
        _, h, w = d.shape
        for i, (l, r, c) in enumerate([(1, 5, 5), (3, h - 6, w - 6), (2, 5, w - 9)]):
            put(d, l, r, c, bump(20.0 + 3 * o + i))
            claims.append((0, (o, l, r, c), "converged", 1))
    add("geometry-octaves", H, W, [a, b], "candidates in the corners of the interior of every octave of a three-octave image",
        claims=claims, kept=[9, 6], candidates=[9, 6])
    # the checkerboard: more than one workgroup row of candidates per segment row, and the overflow input
    for H, W in ((16, 16), (24, 40)):
        n = checkerboard_count(H, W)
        add(f"checkerboard-{H}x{W}", H, W, [checkerboard(H, W), sparse_dog(H, W)], f"{n} keypoints against cap 1024 in image 0, "
            "a sparse image 1 behind it", kept=[n, 2 * len(R.octave_sizes(H, W))], candidates=[n, 2 * len(R.octave_sizes(H, W))])
    return out


def checkerboard_full():
    """the 16 x 16 checkerboard with 16 samples of one row cleared (octave 0, layer 3, row 5, columns 5 .. 20): they stop being
    candidates (v != 0), their neighbours stay extrema and still converge at once (with an offset of 1 / 6 towards the gap), so
    exactly cap = 1024 keypoints are left.  The CPU test asserts the count."""
    dog = checkerboard(16, 16)
    dog[0][3, 5, 5:21] = 0.0
    return dog


# ---------------------------------------------------------------- orient
@dataclass
class OrientCase:
    name: str
    H: int
    W: int
    gauss: List[np.ndarray]                           # [octave] float32 [6, h, w], one image
    ki: np.ndarray                                    # int [n, 4]
    kf: np.ndarray                                    # float64 [n, 4] = x, y, size, response
    edge: str
    peaks: Optional[List[int]] = None                 # peaks per keypoint
    stage: str = "orient"


def _kf(ki, size=1.2):
    ki = np.asarray(ki, dtype=np.int64).reshape(-1, 4)
    kf = np.zeros((len(ki), 4))
    kf[:, 0], kf[:, 1] = ki[:, 3] * 0.5 - 0.25, ki[:, 2] * 0.5 - 0.25
    kf[:, 2] = size
    kf[:, 3] = (np.arange(len(ki)) + 1) / 256.0
    return ki, kf


def _plane(H, W, l, img, o=0):
    g = zero_gauss(H, W)
    g[o][l] = np.asarray(img, dtype=np.float32)
    return g


def valley(h, w, c0, left, right):
    x = np.arange(w, dtype=np.float64) - c0
    return np.tile(np.where(x < 0, -left * x, right * x), (h, 1))


def line(h, w, c0, v=100.0):
    img = np.zeros((h, w))
    img[:, c0] = v
    return img


def dots(h, w, sites):
    img = np.zeros((h, w))
    for y, x, v in sites:
        img[y, x] = v
    return img


def cone(h, w, r0, c0, a=10.0, b=13.0, k=0.37):
    """an elliptic cone, sheared so that no gradient is axis-aligned or diagonal: gradients in every direction around (r0, c0)"""
    y, x = np.meshgrid(np.arange(h, dtype=np.float64) - r0, np.arange(w, dtype=np.float64) - c0, indexing="ij")
    return np.sqrt((a * (x + k * y)) ** 2 + (b * y) ** 2 + 0.731)


def facets(h, w, r0, c0, a0, scale=20.0, n=12):
    """a pyramid of n flat faces around (r0, c0): the gradient is one of n directions a0 + 360 k / n degrees, each over an n-th of
    the plane; 12 faces 30 degrees apart feed every third bin, the densest pattern that the 1 4 6 4 1 smoothing leaves as peaks"""
    y, x = np.meshgrid(np.arange(h, dtype=np.float64) - r0, np.arange(w, dtype=np.float64) - c0, indexing="ij")
    ang = np.radians(a0 + 360.0 / n * np.arange(n))
    return (scale * (x[..., None] * np.cos(ang) + y[..., None] * np.sin(ang))).max(-1)


def ramp(h, w, gx=3.0, gy=1.0):
    y, x = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    return gx * x + gy * y


def orient_cases():
    out = []
    H = W = 16
    h = w = 32
    mid = [(0, 1, 16, 16)]

    def add(name, img, ki, edge, peaks=None, size=1.2, l=1):
        k, f = _kf(ki, size)
        out.append(OrientCase(name, H, W, _plane(H, W, l, img), k, f, edge, peaks))

    add("two-peaks", valley(h, w, 16, 10.0, 9.0), mid, "a valley with slopes 10 and 9: peaks at 180 and 0 degrees, the second at 0.9 of "
        "the first, listed by height and so against bin order", [2])
    add("two-peaks-tie", line(h, w, 16), mid * 3, "a bright column through the keypoint: the bins of 0 and 180 degrees receive the same "
        "terms in the same order, an exact tie that bin order decides; the keypoint repeated three times", [2, 2, 2])
    add("four-tie", dots(h, w, [(16, 16, 100.0)]), mid, "one bright pixel on the keypoint: four equal peaks at 0, 90, 180, 270 degrees, each "
        "bin a single term, kept in bin order", [4])
    add("three", dots(h, w, [(16, 16, 100.0), (15, 16, 100.0)]), mid, "two bright pixels, one above the other: three peaks", [3])
    add("three-distinct", dots(h, w, [(13, 20, 161.0), (15, 20, 50.0), (19, 15, 169.0), (13, 15, 44.0), (13, 16, 100.0), (15, 14, 35.0),
                                      (12, 16, 45.0)]), mid, "seven pixels from a seeded search: three peaks of different heights", [3])
    add("five", dots(h, w, [(17, 12, 130.0), (17, 18, 140.0), (15, 15, 75.0), (15, 13, 120.0), (16, 18, 48.0), (18, 17, 149.0),
                            (19, 12, 27.0)]), mid, "seven pixels from a seeded search: five peaks of different heights", [5])
    add("cone", cone(h, w, 16.31, 15.57, 10.0, 10.0, 0.0), mid, "gradients of one length in every direction: six peaks over the 0.8 line.  "
        "(All 18 local maxima cannot be over it together: the 1 4 6 4 1 smoothing maps an alternating histogram to a constant.)", [6], size=3.0)
    add("facets", facets(h, w, 15.75, 15.85, 11.0), mid, "a twelve-faced pyramid: gradients in twelve directions 30 degrees apart, "
        "eleven peaks of different heights over the 0.8 line, the most of any case (of the 18 SIFT_MAX_PEAKS has room for)", [11], size=3.0)
    add("wrap-to-zero", dots(h, w, [(16, 16, 100.0), (14, 14, 1e-5), (13, 13, 1.76e-6)]), mid, "the four-tie with a gradient of 1e-5 in "
        "bin 35: the peak in bin 0 interpolates to just below 0, wraps to just below 36 bins and rounds to 360.f in float32, which is "
        "reported as 0", [4])
    add("wrap-negative", dots(h, w, [(16, 16, 100.0), (14, 14, 30.0), (13, 13, 5.28)]), mid, "bin 35 higher than bin 1 beside the peak "
        "in bin 0: bn < 0 wraps to an angle in (355, 360)", [4])
    add("wrap-positive", dots(h, w, [(16, 16, 100.0), (14, 14, 30.0), (15, 13, 5.28)]), mid, "the mirror image: bin 1 higher than bin 35, "
        "an angle in (0, 5) and no wrap", [4])
    edge = [(0, 1, 5, 5), (0, 1, 5, w - 6), (0, 1, h - 6, 5), (0, 1, h - 6, w - 6), (0, 1, 5, 16), (0, 1, 16, w - 6)]
    add("cut-windows", cone(h, w, 14.3, 17.7, 7.0, 11.0, -0.29), edge, "keypoints on the first and last interior row and column with a "
        "radius of 9: the window is cut by the y <= 0 / y >= h - 1 / x <= 0 / x >= w - 1 skip", None, size=2.0)
    add("no-gradient", np.full((h, w), 77.0), mid * 2 + edge[:1], "a constant plane: an all-zero histogram has no peak, so the keypoint "
        "gets no orientation and leaves no oriented keypoint", [0, 0, 0])
    add("no-gradient-between", dots(h, w, [(16, 6, 50.0)]) + 77.0,
        [(0, 1, 16, 6), (0, 1, 16, 20), (0, 1, 16, 6)], "a keypoint without gradient between two with four peaks: the scan passes a zero", [4, 0, 4])
    return out


def two_peak_overflow():
    """(H, W, gauss, ki, kf) per image of a B = 2 batch at 8 x 8: image 0 holds cap = 1024 copies of the two-peaks-tie keypoint (2048
    oriented keypoints against cap2 = 1280), image 1 the four-tie keypoint once and a keypoint without gradient"""
    H = W = 8
    k0, f0 = _kf([(0, 1, 8, 8)] * 1024)
    k1, f1 = _kf([(0, 2, 8, 8), (0, 1, 8, 8)])
    return H, W, [_plane(H, W, 1, line(16, 16, 8)), _plane(H, W, 2, dots(16, 16, [(8, 8, 100.0)]))], [k0, k1], [f0, f1]


# ---------------------------------------------------------------- describe
@dataclass
class DescribeCase:
    name: str
    H: int
    W: int
    gauss: List[np.ndarray]
    oi: np.ndarray                                    # int [n, 6]
    of: np.ndarray                                    # float32 [n, 5]
    edge: str
    zero: bool = False
    stage: str = "describe"


def describe_cases():
    out = []
    H = W = 16
    oi = np.array([(0, 1, 16, 16, 0, 0), (0, 1, 5, 5, 0, 1), (0, 1, 26, 26, 1, 1)], dtype=np.int64)
    of = np.array([(7.75, 7.75, 2.0, 0.0, 0.5), (2.25, 2.25, 3.0, 33.0, 0.25), (12.75, 12.75, 1.5, 271.5, 0.125)], dtype=np.float32)
    out.append(DescribeCase("constant", H, W, _plane(H, W, 1, np.full((32, 32), 77.0)), oi, of, "a constant plane: the all-zero histogram, "
                            "the n1 == 0 exit", zero=True))
    for name in ("four-tie", "two-peaks-tie"):
        c = [c for c in orient_cases() if c.name == name][0]
        oi, of, _ = R.orient([g.astype(np.float64) for g in c.gauss], c.ki[:1], c.kf[:1])
        out.append(DescribeCase("axes-" + name, c.H, c.W, c.gauss, oi, of, "gradients exactly along the keypoint's own axes: the "
                                "orientation coordinate of every sample is an integer, its fraction exactly 0"))
    H, W = 97, 131
    sizes = R.octave_sizes(H, W)
    o = len(sizes) - 1
    h, w = sizes[o]
    g = zero_gauss(H, W)
    g[o][:] = np.random.RandomState(97131).randint(0, 256, size=(R.S + 3, h, w)).astype(np.float32)
    sites = [(5, 5), (5, w - 6), (h - 6, 5), (h - 6, w - 6)]
    oi = np.array([(o, 1 + i % 3, r, c, 0, i) for i, (r, c) in enumerate(sites)], dtype=np.int64)
    of = np.array([(c * 2.0 ** (o - 1), r * 2.0 ** (o - 1), 40.0 * 2.0 ** (o - 4), 17.0 + 83.0 * i, 0.1) for i, (r, c) in enumerate(sites)],
                  dtype=np.float32)
    out.append(DescribeCase("corners-smallest-octave", H, W, g, oi, of, f"keypoints in the four interior corners of the {h} x {w} octave with "
                            "a radius far beyond it: the clamp of the radius to the diagonal and the border skip"))
    return out


def describe_radius(c, n):
    """(unclamped radius, diagonal clamp) of oriented keypoint n, as raw_descriptor computes them"""
    o = int(c.oi[n, 0])
    h, w = c.gauss[o].shape[1:]
    hw = 3.0 * float(c.of[n, 2]) * 0.5 / 2.0 ** (o - 1)
    return int(R._round(hw * np.sqrt(2.0) * (R.D + 1) * 0.5)), int(np.sqrt(float(h) * h + float(w) * w))


# ---------------------------------------------------------------- select
@dataclass
class SelectCase:
    name: str
    of: List[np.ndarray]                              # per image float32 [n, 5]
    keys: List[np.ndarray]                            # per image int [n, 5]
    diameter: float
    max_kpts: int
    edge: str
    entries: Optional[List[int]] = None               # NMS neighbour entries per image
    kept: Optional[List[int]] = None                  # kept per image
    overflow: bool = False
    H: int = 8
    W: int = 8
    stage: str = "select"


def _points(xy, resp=None, seed=0):
    """float32 [n, 5] at positions xy with distinct responses (a seeded permutation) unless given"""
    xy = np.asarray(xy, dtype=np.float64).reshape(-1, 2)
    n = len(xy)
    of = np.zeros((n, 5), dtype=np.float32)
    of[:, :2] = xy
    of[:, 2] = 3.0
    of[:, 3] = (np.arange(n) * 37) % 360
    of[:, 4] = (np.random.RandomState(seed).permutation(n) + 1) / (n + 1.0) if resp is None else resp
    return of


def _keys(n, seed=0):
    k = np.zeros((n, 5), dtype=np.int64)
    p = np.random.RandomState(1000 + seed).permutation(max(n, 1))[:n]
    k[:, 0], k[:, 1], k[:, 2], k[:, 3], k[:, 4] = p % 2, 1 + p % 3, 5 + p // 40, 5 + p % 40, p % 4
    return k


def _cluster(n, x, y):
    return np.tile([[x, y]], (n, 1))


def pairs(n):
    return n * (n - 1) // 2


def select_cases():
    out = []
    sparse = _points([(1.0, 1.0), (1.5, 1.0), (6.0, 6.0), (6.0, 1.0), (30.0, 2.0)], seed=5)

    def add(name, ofs, diameter, max_kpts, edge, **kw):
        out.append(SelectCase(name, ofs, [_keys(len(o), i) for i, o in enumerate(ofs)], diameter, max_kpts, edge, **kw))

    add("coincident-286", [_points(_cluster(286, 3.0, 4.0), seed=1)], 9.0, -1, "286 points on one position: 40755 entries, under the 40960 "
        "there is room for; one is kept", entries=[pairs(286)], kept=[1])
    add("coincident-300", [_points(_cluster(300, 3.0, 4.0), seed=2), sparse], 9.0, -1, "300 points on one position: 44850 entries, too many; "
        "image 0 keeps nothing and reports, image 1 is untouched", entries=[pairs(300), 2], kept=[0, 4], overflow=True)
    two = np.concatenate([_cluster(190, 2.0, 2.0), _cluster(215, 20.0, 2.0)])
    add("clusters-exactly-capn", [_points(two, seed=3)], 9.0, -1, "clusters of 190 and 215 points 18 apart: 17955 + 23005 = 40960 entries, "
        "exactly the capacity, which is not an overflow; one of each is kept", entries=[40960], kept=[2])
    three = np.concatenate([_cluster(190, 2.0, 2.0), _cluster(215, 20.0, 2.0), _cluster(2, 2.0, 30.0)])
    add("clusters-capn-plus-1", [_points(three, seed=4), sparse], 9.0, -1, "one pair more: 40961 entries", entries=[40961, 2], kept=[0, 4],
        overflow=True)
    for n in (1, 255, 256, 257, 1280):
        xy = np.stack([(np.arange(n) * 7) % 61, (np.arange(n) * 11) % 53], axis=1) * 0.25
        add(f"distinct-{n}", [_points(xy, seed=10 + n)], -1.0, -1, f"{n} distinct responses, no NMS: the rank loop over "
            f"{-(-n // 256)} tiles of 256" + (", cap2 exactly" if n == 1280 else ""), entries=[0], kept=[n])
    n = 300
    xy = np.stack([(np.arange(n) * 7) % 61, (np.arange(n) * 11) % 53], axis=1) * 0.25
    resp = np.where(np.arange(n) % 3 == 0, 0.75, np.where(np.arange(n) % 3 == 1, 0.5, 0.25)).astype(np.float32)
    for k in (50, 150, 299):
        add(f"equal-run-cut-{k}", [_points(xy, resp)], -1.0, k, f"runs of 100 equal responses, max_keypoints {k} cuts through a run: the key, "
            "then the index decide", entries=[0], kept=[k])
    add("equal-run-nms", [_points(xy, resp)], 3.0, -1, "the same with a radius of 1.5: equal responses meet in the NMS")
    add("empty-beside-many", [_points(np.zeros((0, 2))), _points(xy, seed=7)], 3.0, -1, "an image without oriented keypoints beside one with 300: "
        "min_stack keeps 0")
    return out
