"""tests/patchnet_cases.py on the CPU: under the restatement (tests/patchnet_ref.py) every crafted input reaches the edge it names, and
where a case claims an exact answer the float32 and the float64 restatement agree bit for bit (e32 == 0) and equal the closed form the
case carries.  tests/test_gpu_patchnet_stages.py asks the GPU for equality on exactly those.  No GPU.  Run with -s to see what every
case reaches."""
import math
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import patchnet_cases as C  # noqa: E402
import patchnet_ref as R  # noqa: E402

PYRAMID = {c.name: c for c in C.pyramid_cases()}
EXTRACT = {c.name: c for c in C.extract_cases()}
IMAGES = C.extract_images()
KINDS = ("hardnet", "affnet", "orinet")


def _same(a, b):
    return a.shape == b.shape and torch.equal(a.double(), b.double())


# ---------------------------------------------------------------- pyramid
def test_pyramid_cases_cover_the_shapes():
    shapes = {tuple(c.image.shape[-2:]) for c in PYRAMID.values()}
    assert shapes == {(32, 32), (63, 90), (64, 64), (65, 67), (97, 131), (128, 160), (160, 96)}
    assert {len(c.sizes) for c in PYRAMID.values()} == {1, 2, 3}
    assert any(c.sizes[-1] == (32, 32) for c in PYRAMID.values()) and any(c.image.shape[0] == 3 for c in PYRAMID.values())
    assert C.SIZES[(128, 160)][-1] == (32, 40) and C.SIZES[(97, 131)][-1] == (48, 65) and C.SIZES[(65, 67)][-1] == (32, 33)


@pytest.mark.parametrize("name", list(PYRAMID))
def test_pyramid_case_reaches_its_edge(name):
    c = PYRAMID[name]
    assert c.image.dtype == torch.float32
    lv64, lv32 = R.pyramid(c.image.double()), R.pyramid(c.image)
    assert [tuple(l.shape[-2:]) for l in lv64] == c.sizes == [tuple(l.shape[-2:]) for l in lv32]
    e32 = [(a.double() - b).abs().max().item() for a, b in zip(lv32, lv64)]
    print(f"{name}: levels {c.sizes}, e32 per level {['%.2e' % e for e in e32]} -- {c.edge}")
    for l in c.exact_levels:
        assert e32[l] == 0.0, (name, l, e32[l])
    if c.constant:
        for l, lev in enumerate(lv64):
            assert l in c.exact_levels and torch.equal(lev, c.image[:, :, :1, :1].double().expand_as(lev)), (name, l)
    if name.startswith("batch3"):
        assert not torch.equal(c.image[0], c.image[1]) and not torch.equal(c.image[1], c.image[2])
    if c.is_ramp:
        H, W = c.image.shape[-2:]
        assert H % 2 == 1 and W % 2 == 1 and len(lv64) == 2
        val, ok = C.ramp_level1(H, W)
        assert ok.sum().item() >= 0.7 * ok.numel()
        d = ((lv64[1][0, 0] - val).abs() * ok).max().item()
        print(f"{name}: level 1 against 3 sx + 5 sy on {int(ok.sum())} interior pixels: {d:.2e}")
        assert d <= 1e-12
        assert ((lv64[1][0, 0] - val).abs() * (~ok)).max().item() > 1e-3             # and the border is not the ramp: the reflection shows


def test_impulses_pin_the_reflect_border():
    """level 1 of each impulse against the blur written out with reflected indices (no edge repeat) and 2 x 2 means"""
    c = PYRAMID["impulses-64x64"]
    k = [1.0, 4.0, 6.0, 4.0, 1.0]
    refl = lambda i, n: -i if i < 0 else (2 * n - 2 - i if i >= n else i)
    repeat = lambda i, n: -i - 1 if i < 0 else (2 * n - 1 - i if i >= n else i)
    lv = R.pyramid(c.image.double())[1]
    differs = 0
    for b, (y0, x0) in enumerate(C.IMPULSES_64):
        def blurred(index):
            out = torch.zeros(64, 64, dtype=torch.float64)
            for y in range(max(0, y0 - 2), min(64, y0 + 3)):
                for x in range(max(0, x0 - 2), min(64, x0 + 3)):
                    out[y, x] = sum(k[dy] * k[dx] * 63.0 for dy in range(5) for dx in range(5)
                                    if index(y + dy - 2, 64) == y0 and index(x + dx - 2, 64) == x0) / 256.0
            return F.avg_pool2d(out[None, None], 2)[0, 0]
        assert torch.equal(lv[b, 0], blurred(refl)), (b, y0, x0)
        differs += int(not torch.equal(blurred(refl), blurred(repeat)))
    assert differs == 5                                                # every impulse near a border tells the two reflections apart


# ---------------------------------------------------------------- extract
def _levels(image):
    return R.pyramid(image.double()), R.pyramid(image)


def test_extract_images_have_the_levels_the_cases_need():
    assert [len(R.pyramid(IMAGES[k])) for k in ("two-levels", "pow2", "three-levels", "portrait", "constant3")] == [2, 2, 3, 2, 3]
    corners = IMAGES["two-levels"][0, 0][[0, 0, -1, -1], [0, -1, 0, -1]]
    assert torch.equal(corners * 4, (corners * 4).round())


@pytest.mark.parametrize("name", list(EXTRACT))
def test_extract_case_reaches_its_edge(name):
    c = EXTRACT[name]
    image = IMAGES[c.image]
    assert c.lafs.dtype == torch.float32 and c.lafs.shape[0] == image.shape[0]
    lv64, lv32 = _levels(image)
    level, margin = R.level_of(c.lafs)
    assert all(level[b].tolist() == c.levels for b in range(c.lafs.shape[0])), (name, level.tolist())
    print(f"{name}: levels {c.levels} of {len(lv64)} built, smallest level margin {margin.min().item():.2e} -- {c.edge}")
    for upright in (False, True):
        p64, p32 = R.extract(lv64, c.lafs.double(), upright), R.extract(lv32, c.lafs, upright)
        for i, L in enumerate(c.levels):
            if L >= len(lv64):                                         # not built: zeros, raw and normalised, in both precisions
                for p in (p64, p32, R.normalize_patches(p64), R.normalize_patches(p32)):
                    assert not p[:, i].any()
        if c.closed is not None:
            assert _same(p64, c.closed[upright]) and _same(p32, c.closed[upright]), (name, upright)      # e32 == 0 and the closed form
    if c.closed is not None:
        assert torch.equal(C.kernel_level(c.lafs), level)


def test_crops_are_the_slices_the_issue_names():
    c, img = EXTRACT["crops"], IMAGES["two-levels"][0, 0]
    crop = img[34:66, 24:56]
    k = {l: i for i, l in enumerate(c.labels)}
    raw = c.closed[False][0, :, 0]
    assert torch.equal(raw[k["identity"]], crop) and torch.equal(raw[k["rot90"]], crop.T.flip(1))
    assert torch.equal(raw[k["rot180"]], crop.flip(0).flip(1)) and torch.equal(raw[k["rot270"]], crop.T.flip(0))
    assert torch.equal(raw[k["mirror-x"]], crop.flip(1)) and torch.equal(raw[k["mirror-swap"]], crop.T)
    assert torch.equal(c.closed[True][0, k["rot90"], 0], crop)                       # upright: the rotation is dropped
    ys, xs = torch.arange(34, 66).clamp(0, 95), torch.arange(-11, 21).clamp(0, 127)
    assert torch.equal(raw[k["clamp-left"]], img[ys][:, xs])
    for label, v in (("outside-top-left", 0.5), ("outside-bottom-right", 1.0), ("far-corner", 1.0)):
        assert torch.equal(raw[k[label]], torch.full((32, 32), v)), label
        for p in (raw[k[label]], raw[k[label]].double()):                             # the normalised constant patch is exactly 0
            assert not R.normalize_patches(p[None, None]).any()
    assert torch.equal(raw[k["far-left"]], raw[k["far-left"]][:1].expand(32, 32))     # rot90 far left: x is clamped to 0, y runs along j
    assert all(len({float(v) for v in raw[i].flatten()}) > 900 for l, i in k.items() if l in ("identity", "rot90", "mirror-x", "mirror-swap"))


def test_boundaries_decide_as_the_kernel_does():
    """level_of in float64 on the fp32-valued LAFs and the kernel's halving loop in float32 choose the same level at every boundary,
    with margin 0 on the boundary itself and one fp32 step (8.6e-8 in log2) below it"""
    lafs, levels = C.boundary_lafs()
    level, margin = R.level_of(lafs)
    assert level[0].tolist() == levels == C.kernel_level(lafs)[0].tolist()
    assert sorted(set(levels)) == [0, 1, 2, 3]
    sc = R.scale_of(lafs.double())[0]
    on = [i for i in range(16) if float(sc[i]) in (16.0, 32.0, 64.0, 128.0)]
    assert len(on) == 8 and all(math.log2(2 * float(sc[i]) / 32) == round(math.log2(2 * float(sc[i]) / 32)) for i in on)
    below = [i for i in range(16) if i not in on]
    for i in below:
        s = float(sc[i])
        up = float(torch.nextafter(torch.tensor(s, dtype=torch.float32), torch.tensor(1e9)))
        assert up in (16.0, 32.0, 64.0, 128.0) and s < up
    for name in ("mirrored-level-1", "degenerate", "constant3"):                       # and on the other cases, whose margins are wide
        c = EXTRACT[name]
        got = C.kernel_level(c.lafs)[0].tolist()
        assert got == [min(l, 12) for l in c.levels], (name, got)


def test_degenerate_case():
    c = EXTRACT["degenerate"]
    lv64, lv32 = _levels(IMAGES[c.image])
    img = IMAGES[c.image][0, 0]
    for upright in (False, True):
        p64, p32 = R.extract(lv64, c.lafs.double(), upright)[0, :, 0], R.extract(lv32, c.lafs, upright)[0, :, 0]
        assert torch.equal(p64[0], img[50, 40].double().expand(32, 32)) and torch.equal(p32[0], img[50, 40].expand(32, 32))
        i64 = img.double()                                             # the centre (40.25, 50.75) samples at (39.75, 50.25)
        v = 0.75 * (0.25 * i64[50, 39] + 0.75 * i64[50, 40]) + 0.25 * (0.25 * i64[51, 39] + 0.75 * i64[51, 40])
        assert (p64[1] - v).abs().max().item() <= 1e-15
        assert not p64[3:].any() and not p32[3:].any()
    up = R.extract(lv64, c.lafs.double(), True)[0, 2, 0]
    assert torch.equal(up, img[30, 60].double().expand(32, 32))                        # singular A, upright: scale 0, the centre pixel
    assert len({float(v) for v in R.extract(lv64, c.lafs.double(), False)[0, 2, 0].flatten()}) > 50   # not upright: a line through the image


def test_constant3_case():
    c = EXTRACT["constant3"]
    lv64, lv32 = _levels(IMAGES[c.image])
    for upright in (False, True):
        p, p32 = R.extract(lv64, c.lafs.double(), upright), R.extract(lv32, c.lafs, upright)
        for b in range(3):
            assert (p[b] - (b + 1)).abs().max().item() <= 1e-14
            for q in (p, p32):                                         # the two level-0 LAFs sample pixels: b + 1 exactly, e32 == 0
                assert torch.equal(q[b, :2], torch.full_like(q[b, :2], b + 1.0))
    # levels 1 and 2 are b + 1 up to rounding only: the std of such a patch is rounding noise and its normalisation says nothing
    n32 = R.normalize_patches(R.extract(lv32, c.lafs))
    assert not c.normalised and all(e.normalised for e in EXTRACT.values() if e is not c)
    assert (n32 - R.normalize_patches(R.extract(lv64, c.lafs.double()))).abs().max().item() > 1e-2


# ---------------------------------------------------------------- networks
def _trace_relu(sd, kind, patches):
    """the largest ReLU output of the trunk in float64"""
    x = R.normalize_patches(patches.double())
    worst = 0.0
    for i, stride in zip(R.CONV_IDX, R.STRIDES):
        x = F.conv2d(x, sd[f"features.{i}.weight"].double(), stride=stride, padding=1)
        mean, var = (sd[f"features.{i + 1}.running_{k}"].double().view(1, -1, 1, 1) for k in ("mean", "var"))
        x = (x - mean) / torch.sqrt(var + R.BN_EPS)
        x = F.relu(x)
        worst = max(worst, x.max().item())
    return worst


def test_seam_patches_differ_across_the_chunk():
    idx = C.seam_index(515)
    assert math.gcd(C.SEAM_UNIQUE, C.CHUNK) == 1 and int(idx[512]) != int(idx[0]) and int(idx[513]) != int(idx[1])
    assert all(int(idx[C.CHUNK + i]) != int(idx[i]) for i in range(3))
    u = C.random_patches(C.SEAM_UNIQUE, 50)
    assert all(not torch.equal(u[i], u[j]) for i in range(7) for j in range(i))
    lafs = C.random_lafs(515 + C.EXTRA, 51)
    assert len({tuple(r.flatten().tolist()) for r in lafs}) == 515 + C.EXTRA
    for kind in KINDS:                                                 # the outputs of the 7 differ too, so a row from the wrong patch shows
        r = R.net_forward(C._state_dict(kind), kind, u.double())
        d = (r[:, None] - r[None]).abs().amax(-1) + torch.eye(7)
        assert d.min().item() > 1e-4, (kind, d.min().item())


@pytest.mark.parametrize("kind", KINDS)
def test_dead_trunk_is_dead(kind):
    patches = C.dead_patches()
    assert len(patches) == len(C.UPDATE_LAFS)
    for zero in (True, False):
        sd = C.dead_trunk(kind, tail_mean_zero=zero)
        assert _trace_relu(sd, kind, patches) == 0.0
        r64, r32 = R.net_forward(sd, kind, patches.double()), R.net_forward(sd, kind, patches)
        assert torch.isfinite(r64).all() and torch.isfinite(r32).all()
        if kind == "hardnet" and zero:
            assert not r64.any() and not r32.any()                     # the 1e-12 clamp: 0 / 1e-12, e32 == 0
        elif kind == "hardnet":
            row = -sd["features.20.running_mean"].double() / torch.sqrt(sd["features.20.running_var"].double() + R.BN_EPS)
            assert (r64 - row / row.norm()).abs().max().item() <= 1e-15
        else:
            assert (r64 - torch.tanh(sd["features.19.bias"].double())).abs().max().item() <= 1e-15
    assert _trace_relu(C._state_dict(kind), kind, patches) > 0.1       # the plain weights are alive


def test_chosen_outputs_reach_their_branches():
    """OriNet: the angle atan2(y0 + 1e-8, y1 + 1e-8) of each target, all four quadrants, the axes, 45 degrees at (0, 0), and fp32
    cancellation to hypot 0 at (-1e-8, -1e-8).  AffNet: the targets come out of tanh, (0, 0, 0) keeps scale and orientation,
    bias -4 leaves 1 + y near 7e-4."""
    patches = C.random_patches(len(C.UPDATE_LAFS), 70)
    want = {"quadrant-1": 45.0, "quadrant-2": 135.0, "quadrant-3": -135.0, "quadrant-4": -45.0, "axis+y1": 0.0, "axis-y1": 180.0,
            "axis+y0": 90.0, "axis-y0": -90.0, "zero-45-degrees": 45.0}
    for name, t in C.ORINET_TARGETS.items():
        sd = C.chosen_tanh("orinet", target=t)
        y = R.net_forward(sd, "orinet", patches.double())
        assert (y - torch.tensor(t, dtype=torch.float64)).abs().max().item() <= 1e-7
        if name in want:
            ang = math.degrees(math.atan2(float(y[0, 0]) + 1e-8, float(y[0, 1]) + 1e-8))
            assert abs((ang - want[name] + 180.0) % 360.0 - 180.0) <= 1e-4, (name, ang)
        else:
            y32 = R.net_forward(sd, "orinet", patches)
            s = y32 + torch.tensor(1e-8)
            assert not s.any()                                         # fp32: both sums cancel exactly, hypot is 0
    for name, t in C.AFFNET_TARGETS.items():
        y = R.net_forward(C.chosen_tanh("affnet", target=t), "affnet", patches.double())
        assert (y - torch.tensor(t, dtype=torch.float64)).abs().max().item() <= 1e-7
    for name, b in C.AFFNET_BIASES.items():
        y = R.net_forward(C.chosen_tanh("affnet", bias=b), "affnet", patches)
        assert y.abs().max().item() < 1.0                              # fp32 tanh(4) is not 1: sqrt(u00 u11) is not 0
        u = 1.0 + y.double()
        assert 6e-4 < u.min().item() < 8e-4 if min(b) < 0 else u.min().item() > 1.99
    lafs = C.UPDATE_LAFS.double()
    z = R.affnet_update(lafs, torch.zeros(len(lafs), 3, dtype=torch.float64))
    assert torch.allclose(R.scale_of(z), R.scale_of(lafs), rtol=1e-12, atol=1e-12)
    keep = lafs[:, 0, :2].norm(dim=1) > 0
    assert torch.allclose(torch.atan2(z[keep, 0, 1], z[keep, 0, 0]), torch.atan2(lafs[keep, 0, 1], lafs[keep, 0, 0]), atol=1e-12)
    A = lafs[:, :, :2]
    det = A[:, 0, 0] * A[:, 1, 1] - A[:, 0, 1] * A[:, 1, 0]
    assert (~keep).sum() == 2 and (det < 0).any() and (det == 0).any() and len(C.UPDATE_LABELS) == len(lafs)
