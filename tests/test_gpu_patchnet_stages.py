"""The stages of the DoG + AffNet + OriNet + HardNet extractor (csrc/patchnet.hip) on crafted inputs (tests/patchnet_cases.py;
tests/test_patchnet_cases_cpu.py proves on the CPU that each case reaches the edge it names), each stage called on its own and held
to the float64 restatement (tests/patchnet_ref.py).

One rule, the one of tests/test_gpu_patchnet.py: the restatement also runs in float32 on the CPU, e32 = max |fp32 - fp64| on that
input, and the GPU error against float64 must be <= 4 e32 + 4 fp32 ulps of the output's largest magnitude (_check, which prints the
figures).  Where the CPU test proved e32 == 0 and a closed form, the GPU is asked for equality instead (_exact).  No exemptions.

Pyramid (og_patch_pyramid): 32 x 32 (the copy alone), 63 x 90, 64 x 64 (last level exactly 32), 65 x 67 and 97 x 131 (resize ratios
that are not 2), 128 x 160 (three levels), 160 x 96 (portrait), B = 3; level count and sizes against pyramid_geometry and the
restatement; constants b + 1 and 2^b, impulses at the border and an integer image exactly; ramps at the odd sizes.
Extract (og_patch_extract), raw and normalised, upright both ways, levels from the GPU pyramid of the same test: exact crops at scale
16 (rotations, mirrors, the clamp over every border and corner, patches wholly outside, centres at +-1e4); scales 16, 32, 64, 128 and
one fp32 step below each, where level 2 is built and where it is not (exact zeros); det < 0 on level 1; A = 0, a singular A, scale
1e6; B = 3 constants on levels 0, 1, 2.
Networks (og_patchnet_forward called as _PatchNet.run calls it): n = 512, 513, 515 across the 512-patch chunk and n = 1, 31, 32, 33,
with `out` only, `lafs` only and both; `out` and `lafs` are 8 rows longer than n and those rows must keep their sentinel; every call
runs on a workspace of 0xFF bytes and again zeroed, bit-identical.  The two sites of the input normalisation give the same bits.  A
dead trunk (every ReLU off) gives exact zero HardNet rows through the 1e-12 clamp, the normalised bias row, or tanh(bias).  A zero
tail weight with bias = atanh(target) chooses the tanh outputs: OriNet in all four quadrants, on the axes, at (0, 0) (45 degrees) and
at (-1e-8, -1e-8) (hypotf of 0); AffNet at 0, +-0.9 and bias +-4, on LAFs with a00 = a01 = 0, det < 0, det = 0, a similarity, an
anisotropic A.

Measured on one MI355X, worst GPU max abs error against float64 / e32 of that check:
  pyramid    random images, level 1 or 2: 1.17e-6 / 1.17e-6 (97 x 131); ramp 97 x 131 (values to 870): 8.7e-5 / 9.5e-5; integer image
             level 2: 2.9e-6 / 3.8e-6; every exact level equal
  extract    raw 1.55e-6 / 1.55e-6, normalised 1.33e-5 / 1.64e-5 (boundary LAFs); det < 0 on level 1 5.3e-7 / 8.7e-7; every exact
             crop and every level that is not built equal; the top clamp at height 96 is the crop itself, 3.4e-15 from the
             float64 restatement (whose grid round trip is not exact there)
  HardNet    1.44e-7 / 7.7e-8 (n = 33), dead trunk with a tail mean 3.5e-8 / 3.5e-8
  AffNet     outputs 2.9e-8 / 2.9e-8; LAFs across the chunk 2.8e-6 / 3.4e-6, targets -0.9: 1.8e-5 / 1.4e-5
  OriNet     outputs 2.3e-8 / 4.7e-8; LAFs across the chunk 6.1e-6 / 1.5e-5, chosen angles 7.7e-7 / 7.7e-7
No check exceeded 2 e32 (1.9 e32: HardNet n = 33; 2 e32, one ulp of 3: the B = 3 constants on level 1) but one: the constant patch
of A = 0 at a fractional centre, a single bilinear value, is 4.8e-8 (0.8 ulp) from float64 where the float32 restatement happens to
be 1.1e-8 from it, and passes on the 4 ulp term of the rule.  Two chosen outputs are ill-conditioned in the restatement itself, so
the rule holds them only loosely; they are kept for the branch they reach and for finiteness:
  AffNet bias -4: 1 + y is 6.7e-4 and carries the rounding of tanhf (3e-8), which sqrt(u00 u11) in the denominator turns into
             0.51 on LAF entries near 1e4 (GPU 0.512 / e32 0.513).
  OriNet (-1e-8, -1e-8): y + 1e-8f is exactly 0 in fp32, on the GPU and in the float32 restatement (no rotation); in float64 the
             sums are the rounding of 1e-8f, 6e-17 each, and the angle is 45 degrees: e32 = 9.4, the size of the LAF.
A bias at which fp32 tanh returns exactly +-1 makes sqrt(u00 u11) zero in every fp32 reading; no case goes there.

What the file found: nothing in patchnet.hip; every case passes on the unchanged source.  It found two things about the checks.  The
float64 restatement is not the crop at the top rows of an image whose height is no power of two (above).  And the normalisation of a
patch that is constant up to rounding (B = 3 constants on level 1 and 2) is noise of size 0.2 on both sides, so that case is not
compared normalised (proved on the CPU).

Single-line changes of patchnet.hip tried on a scratch copy, each built as a library of its own and run on an MI355X against this file
(77 tests) and tests/test_gpu_patchnet.py (13 tests), each in a process of its own; the unchanged source passes all 90.  What failed
here, and in brackets what failed there:
  1  `c0` dropped from `pc`                   test_chunk_seam[*-513, *-515], all three kinds                                          [none]
  2  `c0` dropped from `oc`                   test_chunk_seam[hardnet-513, hardnet-515]                                               [none]
  3  `c0` dropped from `lc`                   test_chunk_seam[affnet-513, affnet-515, orinet-513, orinet-515]                         [none]
  4  `c0` dropped from the `raw` pointers     test_chunk_seam[affnet-513, affnet-515, orinet-513, orinet-515]                         [none]
  5  pn_reflect `2 * n - 2 - i` -> `- 1 -`    test_pyramid[every random image of two or more levels, batch3, impulses, integers, both ramps],
                                              test_extract[boundaries-*, mirrored-level-1-False]   [test_pyramid_and_extract, test_end_to_end]
  6  `t >= 2.f` -> `t > 2.f`                  test_extract[boundaries-three-levels-*, boundaries-two-levels-*, mirrored-level-1-*]    [none]
  7  `min(hl, wl)` -> `hl` in `r`             test_extract[crops-portrait-False, crops-portrait-True]                                 [none]
  8  `fabsf` removed in pn_extract_kernel     test_extract[crops-True, crops-portrait-True, crops-pow2-True, mirrored-level-1-*]      [none]
     `fabsf` removed in pn_tail_laf_kernel    test_chunk_seam[affnet-*], test_small_n[affnet-31, -32, -33], test_dead_trunk[affnet],
                                              test_affnet_chosen_outputs[all]                                       [test_each_net[*-affnet]]
  9  `a01` and `a10` swapped in the sampler   test_extract[crops-False, crops-portrait-False, crops-pow2-False, clamp-top-96-False,
                                              boundaries-*-False, mirrored-level-1-False]          [test_pyramid_and_extract, test_end_to_end]
 10  `1.f / 1023.f` -> `1.f / 1024.f`         test_extract[all but constant3 and degenerate-True], test_chunk_seam[all], test_small_n[all]
                                                                                   [test_pyramid_and_extract, test_each_net[all], test_end_to_end]
 11  resize `+ 0.5f` -> `+ 0.f`               test_pyramid[as for 5], test_extract[boundaries-*, mirrored-level-1-*]
                                                                                                   [test_pyramid_and_extract, test_end_to_end]
 12  `1e-12f` -> `0.f` in pn_l2norm_kernel    test_dead_trunk[hardnet]                                                                [none]
 13  `sn` / `cs` swapped in the OriNet branch test_chunk_seam[orinet-*], test_small_n[orinet-*], test_dead_trunk[orinet],
                                              test_orinet_chosen_outputs[quadrant-2, quadrant-4, the four axes]
                                              (quadrants 1 and 3 and (0, 0) lie on the diagonal the swap maps to itself)
                                                                                                   [test_each_net[*-orinet], test_end_to_end]
 14  `h > 0.f ? a00 / h : 1.f` -> `a00 / h`   test_dead_trunk[affnet], test_affnet_chosen_outputs[all]                                [none]
 15  not run, because they read or write past a buffer: `lev < g.levels` -> `<=`, the tail's `min(p0 + (lane & 31), n - 1)`, and the
     removal of a `patch < n` / `p0 + m >= n` / `p >= n` guard.  The sentinel rows and the 0xFF workspace are what would show them.
"""
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import patchnet_cases as C  # noqa: E402
import patchnet_ref as R  # noqa: E402

from openglue_amd import _lib  # noqa: E402
from openglue_amd.affnet_hardnet import KINDS as KIND_ID, AffNet, HardNet, OriNet, PatchPyramid, pyramid_geometry  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
ULP = 2.0 ** -23
NETS = {"hardnet": HardNet, "affnet": AffNet, "orinet": OriNet}
PYRAMID = {c.name: c for c in C.pyramid_cases()}
EXTRACT = {c.name: c for c in C.extract_cases()}
IMAGES = C.extract_images()
UPDATE = {"affnet": R.affnet_update, "orinet": R.orinet_update}


def _check(name, got, ref64, ref32):
    """GPU `got` against float64 under the tolerance rule of test_gpu_patchnet.py; prints the figures before it asserts"""
    got = got.detach().cpu().double()
    assert got.shape == ref64.shape, (name, got.shape, ref64.shape)
    assert torch.isfinite(got).all(), name
    e32 = (ref32.double() - ref64).abs().max().item() if ref64.numel() else 0.0
    err = (got - ref64).abs().max().item() if ref64.numel() else 0.0
    floor = 4 * ULP * (ref64.abs().max().item() if ref64.numel() else 0.0)
    print(f"patchnet stages {name}: GPU max |d| {err:.3e}, e32 {e32:.3e}, bound {4 * e32 + floor:.3e}")
    assert err <= 4 * e32 + floor, (name, err, e32, floor)
    return err, e32


def _exact(name, got, want):
    """equality, where tests/test_patchnet_cases_cpu.py proved e32 == 0"""
    got = got.detach().cpu()
    assert got.shape == want.shape, (name, got.shape, want.shape)
    bad = int((got != want).sum())
    print(f"patchnet stages {name}: exact, {bad} of {want.numel()} values differ")
    assert torch.equal(got, want), (name, bad, (got.double() - want.double()).abs().max().item())


# ---------------------------------------------------------------- pyramid
@functools.lru_cache(maxsize=None)
def _pyramid_reference(key, kind="pyramid"):
    image = PYRAMID[key].image if kind == "pyramid" else IMAGES[key]
    return R.pyramid(image.double()), R.pyramid(image)


@pytest.mark.parametrize("name", list(PYRAMID))
def test_pyramid(name):
    c = PYRAMID[name]
    B, _, H, W = c.image.shape
    lv64, lv32 = _pyramid_reference(name)
    sizes, floats = pyramid_geometry(H, W)
    assert sizes == c.sizes == [tuple(l.shape[-2:]) for l in lv64] and floats == sum(h * w for h, w in sizes)
    pyr = PatchPyramid(c.image.to(DEV))
    got = pyr.levels
    assert [tuple(l.shape) for l in got] == [(B, 1, h, w) for h, w in sizes]
    assert pyr.buffer.numel() == B * floats
    for l in range(len(sizes)):
        if l in c.exact_levels:
            _exact(f"pyramid {name} level {l}", got[l], lv32[l])
        else:
            _check(f"pyramid {name} level {l}", got[l], lv64[l], lv32[l])
        if c.constant:
            assert torch.equal(got[l].cpu(), c.image[:, :, :1, :1].expand(B, 1, *sizes[l])), (name, l)
    assert torch.equal(PatchPyramid(c.image.to(DEV)).buffer, pyr.buffer)


# ---------------------------------------------------------------- extract
def _constant_rows(p64):
    flat = p64.flatten(2)
    return flat.amax(-1) == flat.amin(-1)                              # [B, N]


@pytest.mark.parametrize("upright", [False, True])
@pytest.mark.parametrize("name", list(EXTRACT))
def test_extract(name, upright):
    c = EXTRACT[name]
    image = IMAGES[c.image]
    lv64, lv32 = _pyramid_reference(c.image, "extract")
    pyr = PatchPyramid(image.to(DEV))
    lafs = c.lafs.to(DEV)
    tag = f"extract {name} upright={upright}"
    p64, p32 = R.extract(lv64, c.lafs.double(), upright), R.extract(lv32, c.lafs, upright)
    raw = pyr.extract(lafs, upright=upright)
    nrm = pyr.extract(lafs, upright=upright, normalize=True)
    assert raw.shape == nrm.shape == p64.shape
    if c.closed is not None:
        _exact(tag, raw, c.closed[upright])
    else:
        _check(tag, raw, p64, p32)
    missing = [i for i, L in enumerate(c.levels) if L >= len(lv64)]    # the level is not built: exact zeros, raw and normalised
    if missing:
        _exact(tag + " levels not built", raw[:, missing], torch.zeros(raw.shape[0], len(missing), 1, 32, 32))
        _exact(tag + " levels not built, normalised", nrm[:, missing], torch.zeros(raw.shape[0], len(missing), 1, 32, 32))
    # normalised: the constant patches apart, as test_gpu_patchnet.py does (their float32 CPU mean need not be exact)
    n64, n32 = R.normalize_patches(p64), R.normalize_patches(p32)
    const = _constant_rows(p64)
    for what, rows in (("normalised", ~const), ("normalised, constant patches", const)):
        if rows.any() and c.normalised:
            _check(f"{tag} {what}", nrm.cpu()[rows], n64[rows], n32[rows])
    if name == "crops":                                                # corner pixels are multiples of 0.25: proved exactly 0 on the CPU
        k = [c.labels.index(l) for l in ("outside-top-left", "outside-bottom-right", "far-corner")]
        _exact(tag + " normalised constant patch", nrm[:, k], torch.zeros(1, 3, 1, 32, 32))
    if name == "constant3":
        for b in range(3):                                             # level 0 samples pixels: b + 1 exactly
            assert torch.equal(raw[b, :2].cpu(), torch.full((2, 1, 32, 32), b + 1.0)), b


# ---------------------------------------------------------------- networks
def _net(kind, sd=None):
    net = NETS[kind]()
    sd = C._state_dict(kind) if sd is None else sd
    net.load_state_dict(sd, strict=True)
    return net.eval().to(DEV), sd


def _bits(t):
    return t.view(torch.int32)


def _forward(net, kind, x, n, lafs=None, want_out=True, normalize=True):
    """og_patchnet_forward called as _PatchNet.run calls it, on n patches, with `out` and `lafs` EXTRA rows longer than n and holding
    a sentinel there; twice on one workspace of exactly the size asked for, filled with 0xFF bytes (NaN) and then zeroed.  The two
    answers must be bit-identical and the sentinel rows untouched.  -> out [n, width] or None, lafs [n, 2, 3] or None, on the CPU"""
    assert x.shape == (n, 1, 32, 32) and (lafs is None or lafs.shape == (n, 2, 3))
    xd = x.to(DEV).contiguous()
    nbytes = _lib.load().og_patch_workspace_bytes(0, 0, 0, n)
    assert nbytes > 0
    ws = torch.empty(nbytes, device=DEV, dtype=torch.uint8)
    width = C.WIDTH[kind]
    runs = []
    for fill in (0xFF, 0x00):
        ws.fill_(fill)
        out = torch.full((n + C.EXTRA, width), C.SENTINEL, device=DEV) if want_out else None
        lb = None
        if lafs is not None:
            lb = torch.full((n + C.EXTRA, 2, 3), C.SENTINEL, device=DEV)
            lb[:n] = lafs.to(DEV)
        _lib.call("og_patchnet_forward", DEV, KIND_ID[kind], n, xd.data_ptr(), int(normalize), net._pack(DEV).data_ptr(), _lib.ptr(out),
                  _lib.ptr(lb), ws.data_ptr(), _lib.STREAM)
        torch.cuda.synchronize()
        runs.append((out, lb))
    for a, b in zip(*runs):
        if a is not None:
            assert torch.equal(_bits(a), _bits(b)), (kind, n, "the answer depends on what the workspace held")
            assert bool((a[n:] == C.SENTINEL).all()), (kind, n, "rows behind n were written")
    out, lb = runs[0]
    return (None if out is None else out[:n].cpu()), (None if lb is None else lb[:n].cpu())


@functools.lru_cache(maxsize=None)
def _reference(kind, which):
    """the restatement on the unique patches of a group, once per kind: (patches, r64, r32)"""
    patches = C.random_patches(C.SEAM_UNIQUE, 50) if which == "seam" else C.random_patches(max(C.SMALL_N), 52)
    sd = C._state_dict(kind)
    return patches, R.net_forward(sd, kind, patches.double()), R.net_forward(sd, kind, patches)


def _net_case(kind, n, which):
    net, _ = _net(kind)
    patches, r64, r32 = _reference(kind, which)
    idx = C.seam_index(n) if which == "seam" else torch.arange(n)
    x, r64, r32 = patches[idx], r64[idx], r32[idx]
    tag = f"{kind} n={n}"
    out, _ = _forward(net, kind, x, n)
    _check(tag, out, r64, r32)
    if kind == "hardnet":
        assert ((out.double().norm(dim=1) - 1).abs() < 1e-5).all()
        return
    lafs = C.random_lafs(n, 51)
    l64, l32 = UPDATE[kind](lafs.double(), r64), UPDATE[kind](lafs, r32)
    none, only = _forward(net, kind, x, n, lafs=lafs, want_out=False)
    both_out, both = _forward(net, kind, x, n, lafs=lafs)
    assert none is None and torch.equal(_bits(both_out), _bits(out)) and torch.equal(_bits(both), _bits(only)), tag
    _check(tag + " lafs", both, l64, l32)
    assert torch.equal(both[:, :, 2], lafs[:, :, 2]), tag


@pytest.mark.parametrize("n", C.SEAM_N)
@pytest.mark.parametrize("kind", list(NETS))
def test_chunk_seam(kind, n):
    """n patches that repeat with period 7 across the 512-patch chunk: row 512 + i is another patch than row i, and every LAF differs"""
    _net_case(kind, n, "seam")


@pytest.mark.parametrize("n", C.SMALL_N)
@pytest.mark.parametrize("kind", list(NETS))
def test_small_n(kind, n):
    _net_case(kind, n, "small")


@pytest.mark.parametrize("kind", list(NETS))
def test_the_two_normalisation_sites_agree(kind):
    """pn_normalize4 in the extraction and in conv0: the same bits, a constant patch included"""
    net, _ = _net(kind)
    pyr = PatchPyramid(IMAGES["two-levels"].to(DEV))
    lafs = torch.cat([EXTRACT["crops"].lafs, EXTRACT["degenerate"].lafs, EXTRACT["boundaries-two-levels"].lafs], 1).to(DEV)
    n = lafs.shape[1]
    raw, nrm = pyr.extract(lafs), pyr.extract(lafs, normalize=True)
    assert bool((raw.flatten(2).amax(-1) == raw.flatten(2).amin(-1)).any())               # a constant patch is among them
    la, lb = (lafs[0].clone(), lafs[0].clone()) if kind != "hardnet" else (None, None)
    a = net.run(nrm, la, normalize=False)
    b = net.run(raw, lb, normalize=True)
    assert a.shape == (n, C.WIDTH[kind]) and torch.isfinite(a).all()
    assert torch.equal(_bits(a), _bits(b))
    if kind != "hardnet":
        assert torch.equal(_bits(la), _bits(lb)) and not torch.equal(la, lafs[0])


@pytest.mark.parametrize("kind", list(NETS))
def test_dead_trunk(kind):
    """every ReLU is off: the 8 x 8 convolution sees zeros.  HardNet with a zero tail mean gives exact zero rows through the 1e-12
    clamp of the L2 normalisation; otherwise the output is the normalised bias row, or tanh(bias)"""
    patches = C.dead_patches()
    n = len(patches)
    for zero in (True, False):
        net, sd = _net(kind, C.dead_trunk(kind, tail_mean_zero=zero))
        r64, r32 = R.net_forward(sd, kind, patches.double()), R.net_forward(sd, kind, patches)
        out, _ = _forward(net, kind, patches, n)
        assert torch.isfinite(out).all()
        if kind == "hardnet" and zero:
            _exact("hardnet dead trunk, zero tail mean", out, torch.zeros(n, 128))
        else:
            _check(f"{kind} dead trunk", out, r64, r32)
        if kind == "hardnet" or zero:
            continue
        lafs = C.UPDATE_LAFS[:n]
        _, got = _forward(net, kind, patches, n, lafs=lafs, want_out=False)
        _check(f"{kind} dead trunk lafs", got, UPDATE[kind](lafs.double(), r64), UPDATE[kind](lafs, r32))


def _chosen(kind, name, sd):
    net, _ = _net(kind, sd)
    lafs = C.UPDATE_LAFS
    n = len(lafs)
    patches = C.random_patches(n, 70)
    r64, r32 = R.net_forward(sd, kind, patches.double()), R.net_forward(sd, kind, patches)
    out, got = _forward(net, kind, patches, n, lafs=lafs)
    _check(f"{kind} {name}", out, r64, r32)
    assert torch.isfinite(got).all(), name
    _check(f"{kind} {name} lafs", got, UPDATE[kind](lafs.double(), r64), UPDATE[kind](lafs, r32))
    assert torch.equal(got[:, :, 2], lafs[:, :, 2])


@pytest.mark.parametrize("name", list(C.ORINET_TARGETS))
def test_orinet_chosen_outputs(name):
    _chosen("orinet", name, C.chosen_tanh("orinet", target=C.ORINET_TARGETS[name]))


@pytest.mark.parametrize("name", list(C.AFFNET_TARGETS) + list(C.AFFNET_BIASES))
def test_affnet_chosen_outputs(name):
    sd = C.chosen_tanh("affnet", target=C.AFFNET_TARGETS[name]) if name in C.AFFNET_TARGETS else C.chosen_tanh("affnet", bias=C.AFFNET_BIASES[name])
    _chosen("affnet", name, sd)
