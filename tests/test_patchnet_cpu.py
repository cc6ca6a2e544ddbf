"""The float64 restatement of the DoG + AffNet + OriNet + HardNet extractor (tests/patchnet_ref.py) against constructions it did not
produce (literal nn.Sequential stacks, another formulation of the sampler), and the boundary of the HIP implementation: state-dict
keys, exported symbols, header, argument checks.  No GPU."""
import os
import re
import sys

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import patchnet_ref as R  # noqa: E402

from openglue_amd import _lib, build as og_build, synthetic as syn  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["og_patch_geometry", "og_patch_workspace_bytes", "og_patch_pyramid", "og_patch_extract", "og_patchnet_packed_bytes",
         "og_patchnet_pack", "og_patchnet_forward"]
KINDS = ("hardnet", "affnet", "orinet")


def _literal(kind):
    """the network written out layer by layer, as kornia does"""
    c = 32 if kind == "hardnet" else 16
    f = [nn.Conv2d(1, c, 3, padding=1, bias=False), nn.BatchNorm2d(c, affine=False), nn.ReLU(),
         nn.Conv2d(c, c, 3, padding=1, bias=False), nn.BatchNorm2d(c, affine=False), nn.ReLU(),
         nn.Conv2d(c, 2 * c, 3, stride=2, padding=1, bias=False), nn.BatchNorm2d(2 * c, affine=False), nn.ReLU(),
         nn.Conv2d(2 * c, 2 * c, 3, padding=1, bias=False), nn.BatchNorm2d(2 * c, affine=False), nn.ReLU(),
         nn.Conv2d(2 * c, 4 * c, 3, stride=2, padding=1, bias=False), nn.BatchNorm2d(4 * c, affine=False), nn.ReLU(),
         nn.Conv2d(4 * c, 4 * c, 3, padding=1, bias=False), nn.BatchNorm2d(4 * c, affine=False), nn.ReLU(),
         nn.Dropout(0.3)]
    if kind == "hardnet":
        f += [nn.Conv2d(4 * c, 128, 8, bias=False), nn.BatchNorm2d(128, affine=False)]
    else:
        f += [nn.Conv2d(4 * c, 3 if kind == "affnet" else 2, 8, bias=True), nn.Tanh()]
    return nn.Sequential(*f)


@pytest.mark.parametrize("kind", KINDS)
def test_functional_reference_equals_the_literal_stack(kind):
    sd = syn.make_patchnet_state_dict(kind, seed=3)
    net = _literal(kind).double().eval()
    net.load_state_dict({k[len("features."):]: v.double() if v.is_floating_point() else v for k, v in sd.items()}, strict=True)
    g = torch.Generator().manual_seed(5)
    patches = torch.rand(5, 1, 32, 32, generator=g, dtype=torch.float64)
    patches[4] = 0.25                                                  # std 0
    with torch.no_grad():
        flat = patches.flatten(1)
        x = (patches - flat.mean(1).view(-1, 1, 1, 1)) / (flat.std(1).view(-1, 1, 1, 1) + 1e-6)
        want = net(x).flatten(1)
        if kind == "hardnet":
            want = F.normalize(want, dim=1)
    got = R.net_forward(sd, kind, patches)
    assert got.shape == want.shape and torch.isfinite(got).all()
    assert (got - want).abs().max().item() <= 1e-12


def test_sampler_equals_another_formulation():
    """one LAF per level (and one whose level is not built): the reference samples through grid_sample(align_corners=False) at
    (2 p + 1) / size - 1; the same pixel positions p through align_corners=True at 2 p / (size - 1) - 1, clamped by hand"""
    image = syn.make_image(96, 128, seed=2).double()
    levels = R.pyramid(image)
    assert [tuple(l.shape[-2:]) for l in levels] == [(96, 128), (48, 64)]
    lafs = torch.tensor([[[[9.0, 3.0, 40.2], [-2.0, 11.0, 30.7]],          # scale 10.2: level 0
                          [[40.0, 12.0, 70.5], [-9.0, 44.0, 50.1]],         # scale 43.2: level 1
                          [[90.0, 0.0, 60.0], [0.0, 90.0, 40.0]],           # level 2: not built
                          [[7.0, 0.0, 1.5], [0.0, 7.0, 95.9]]]], dtype=torch.float64)   # hangs over two borders
    level, margin = R.level_of(lafs)
    assert level[0].tolist() == [0, 1, 2, 0] and margin.min().item() > 0.05
    got = R.extract(levels, lafs)
    assert torch.equal(got[0, 2], torch.zeros(1, 32, 32, dtype=torch.float64))
    for i in (0, 1, 3):
        L = int(level[0, i])
        hl, wl = levels[L].shape[-2:]
        p = R.sample_positions(lafs[0, i], (96, 128), (hl, wl))
        px, py = p[..., 0].clamp(0, wl - 1), p[..., 1].clamp(0, hl - 1)
        grid = torch.stack([2 * px / (wl - 1) - 1, 2 * py / (hl - 1) - 1], -1)[None]
        want = F.grid_sample(levels[L], grid, mode="bilinear", padding_mode="border", align_corners=True)[0]
        assert (got[0, i] - want).abs().max().item() <= 1e-12, i
    up = R.extract(levels, lafs, upright=True)
    s = R.scale_of(lafs[0, 0])
    same = R.extract(levels, torch.tensor([[[[s, 0.0, 40.2], [0.0, s, 30.7]]]], dtype=torch.float64))
    assert torch.equal(up[0, 0], same[0, 0])


def test_pyramid_halves_even_images_by_2x2_means_of_the_blur():
    image = syn.make_image(64, 96, seed=4).double()
    levels = R.pyramid(image)
    assert [tuple(l.shape[-2:]) for l in levels] == [(64, 96), (32, 48)]
    k = torch.tensor([1.0, 4.0, 6.0, 4.0, 1.0], dtype=torch.float64) / 16
    x = F.pad(image, (2, 2, 2, 2), mode="reflect")
    blur = F.conv2d(x, (k[:, None] * k[None, :]).view(1, 1, 5, 5))
    assert (levels[1] - F.avg_pool2d(blur, 2)).abs().max().item() <= 1e-13


def test_laf_updates_keep_scale_and_centre():
    g = torch.Generator().manual_seed(1)
    lafs = torch.randn(6, 2, 3, generator=g, dtype=torch.float64) * 5
    a = R.affnet_update(lafs, torch.tanh(torch.randn(6, 3, generator=g, dtype=torch.float64)))
    o = R.orinet_update(a, torch.tanh(torch.randn(6, 2, generator=g, dtype=torch.float64)))
    for out in (a, o):
        assert torch.allclose(R.scale_of(out), R.scale_of(lafs), rtol=1e-12) and torch.equal(out[..., 2], lafs[..., 2])
    # zero outputs: AffNet gives scale * rot(ori), a similarity with the orientation kept
    z = R.affnet_update(lafs, torch.zeros(6, 3, dtype=torch.float64))
    assert torch.allclose(torch.atan2(z[:, 0, 1], z[:, 0, 0]), torch.atan2(lafs[:, 0, 1], lafs[:, 0, 0]), atol=1e-12)
    assert torch.allclose(z[:, 0, 0], z[:, 1, 1], atol=1e-12) and torch.allclose(z[:, 0, 1], -z[:, 1, 0], atol=1e-12)


def _expected_keys(prefix, kind):
    c = 32 if kind == "hardnet" else 16
    nout = {"hardnet": 128, "affnet": 3, "orinet": 2}[kind]
    shapes = {}
    for i, (cin, cout) in zip((0, 3, 6, 9, 12, 15), [(1, c), (c, c), (c, 2 * c), (2 * c, 2 * c), (2 * c, 4 * c), (4 * c, 4 * c)]):
        shapes[f"{prefix}features.{i}.weight"] = (cout, cin, 3, 3)
        shapes[f"{prefix}features.{i + 1}.running_mean"] = (cout,)
        shapes[f"{prefix}features.{i + 1}.running_var"] = (cout,)
        shapes[f"{prefix}features.{i + 1}.num_batches_tracked"] = ()
    shapes[f"{prefix}features.19.weight"] = (nout, 4 * c, 8, 8)
    if kind == "hardnet":
        shapes[f"{prefix}features.20.running_mean"] = (128,)
        shapes[f"{prefix}features.20.running_var"] = (128,)
        shapes[f"{prefix}features.20.num_batches_tracked"] = ()
    else:
        shapes[f"{prefix}features.19.bias"] = (nout,)
    return shapes


def test_state_dict_keys_and_shapes():
    from openglue_amd.affnet_hardnet import AffNet, DoGAffNetHardNet, HardNet, OriNet
    want = {}
    for prefix, kind in (("hardnet.", "hardnet"), ("affnet.", "affnet"), ("orinet.angle_detector.", "orinet")):
        want.update(_expected_keys(prefix, kind))
    model = DoGAffNetHardNet()
    got = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    assert got == want
    full = {}
    for prefix, kind in (("hardnet.", "hardnet"), ("affnet.", "affnet"), ("orinet.angle_detector.", "orinet")):
        full.update({prefix + k: v for k, v in syn.make_patchnet_state_dict(kind, seed=0).items()})
    model.load_state_dict(full, strict=True)
    with pytest.raises(RuntimeError):
        model.load_state_dict({k: v for k, v in full.items() if k != "affnet.features.19.bias"}, strict=True)
    for cls, kind in ((HardNet, "hardnet"), (AffNet, "affnet"), (OriNet, "orinet")):
        sd = syn.make_patchnet_state_dict(kind, seed=1)
        assert {k: tuple(v.shape) for k, v in sd.items()} == _expected_keys("", kind)
        cls().load_state_dict(sd, strict=True)
        assert all(torch.equal(a, b) for a, b in zip(sd.values(), syn.make_patchnet_state_dict(kind, seed=1).values()))
        bn = sd["features.1.running_var"]
        assert 0.75 <= bn.min().item() and bn.max().item() <= 1.25 and sd["features.1.running_mean"].abs().max().item() > 0


def test_header_and_binding_hold_the_new_entries():
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "openglue_amd.h")).read()
    declared = set(re.findall(r"^\s*(?:int|size_t)\s+(og_\w+)\s*\(", header, flags=re.M))
    for name in NAMES:
        assert name in declared and name in _lib.SYMBOLS and hasattr(lib, name), name
    assert re.search(r"#define OG_ABI_VERSION 14\b", header) and _lib.OG_ABI_VERSION == 14 and lib.og_abi_version() == 14   # additive
    assert "patchnet.hip" in og_build.SOURCES


def test_geometry_packing_and_limits():
    import ctypes as C
    from openglue_amd import affnet_hardnet as ah
    lib = _lib.load()
    for H, W in ((96, 128), (120, 160), (480, 640), (97, 131), (31, 200)):
        sizes, floats = ah.pyramid_geometry(H, W)
        assert sizes == [tuple(l.shape[-2:]) for l in R.pyramid(torch.zeros(1, 1, H, W))]
        assert floats == sum(h * w for h, w in sizes)
    assert lib.og_patch_workspace_bytes(2, 96, 128, 0) >= 2 * 96 * 128 * 4
    assert lib.og_patch_workspace_bytes(0, 0, 0, 65) >= 2 * 65 * 1024 * 32 * 4
    assert lib.og_patch_workspace_bytes(1, 9000, 64, 0) == 0 and lib.og_patch_workspace_bytes(0, 0, 0, -1) == 0
    assert lib.og_patch_pyramid(1, 64, 64, None, None, None, None) == -1                          # OG_E_INVALID
    assert lib.og_patch_extract(1, 64, 64, 3, None, None, 0, 0, None, None) == -1
    assert lib.og_patchnet_forward(7, 1, None, 0, None, None, None, None, None) == -2             # OG_E_SHAPE: no such net
    assert lib.og_patchnet_packed_bytes(7) == 0
    # the packed blob holds every folded weight once: sizes, and a non-finite fold is refused
    for kind, k in ah.KINDS.items():
        c = 32 if kind == "hardnet" else 16
        nout = {"hardnet": 128, "affnet": 3, "orinet": 2}[kind]
        convs = [(c, c), (c, 2 * c), (2 * c, 2 * c), (2 * c, 4 * c), (4 * c, 4 * c)]
        want = 10 * c + sum(max(co, 32) * (9 * ci + 1) for ci, co in convs) + nout * 64 * 4 * c + (nout + 3) // 4 * 4
        assert lib.og_patchnet_packed_bytes(k) == 4 * want
        net = {"hardnet": ah.HardNet, "affnet": ah.AffNet, "orinet": ah.OriNet}[kind]()
        net.load_state_dict(syn.make_patchnet_state_dict(kind, seed=0), strict=True)
        host = [t.detach().float().contiguous() for t in net._pack_tensors()]
        ptrs = (C.c_void_p * len(host))(*[h.data_ptr() for h in host])
        blob = torch.zeros(want, dtype=torch.float32)
        assert lib.og_patchnet_pack(k, 1e-5, ptrs, blob.data_ptr()) == 0
        w0 = host[0].double().view(c, 9) / torch.sqrt(host[2].double() + 1e-5)[:, None]
        assert torch.equal(blob[:9 * c].view(9, c), w0.T.float())
        assert torch.equal(blob[9 * c:10 * c], (-host[1].double() / torch.sqrt(host[2].double() + 1e-5)).float())
        host[2][0] = -1.0                                              # var + eps < 0: the fold is NaN
        assert lib.og_patchnet_pack(k, 1e-5, ptrs, blob.data_ptr()) == -5                         # OG_E_RANGE


def test_modules_raise_on_cpu_tensors():
    from openglue_amd.affnet_hardnet import AffNet, DoGAffNetHardNet, HardNet, OriNet, PatchPyramid, extract_patches
    for cls in (HardNet, AffNet, OriNet):
        with pytest.raises(RuntimeError):
            cls().eval()(torch.zeros(2, 1, 32, 32))
    with pytest.raises(RuntimeError):
        DoGAffNetHardNet()(torch.zeros(1, 1, 64, 64))
    with pytest.raises(ValueError):
        DoGAffNetHardNet()(torch.zeros(1, 3, 64, 64))
    with pytest.raises(RuntimeError):
        PatchPyramid(torch.zeros(1, 1, 64, 64))
    with pytest.raises(RuntimeError):
        extract_patches(torch.zeros(1, 1, 64, 64), torch.zeros(1, 2, 2, 3))
