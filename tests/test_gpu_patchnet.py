"""DoG + AffNet + OriNet + HardNet on the MI355X (openglue_amd/affnet_hardnet.py, csrc/patchnet.hip) against the float64 restatement
(tests/patchnet_ref.py).

Tolerance rule, the same in every test: the restatement is also run in float32 on the CPU, e32 = max |fp32 - fp64| on that input; the
GPU error against float64 must be <= 4 e32 + 4 fp32 ulps of the output's largest magnitude.  Nothing is fixed in advance.
Exemption rule (end to end only): a keypoint whose float64 level margin |log2(2 scale / 32) - nearest integer| is below 1e-4 at any of
the three extractions may differ; exemptions are counted with parity_note and must stay <= max(1, 0.5 %) of keypoints.

Measured on one MI355X, GPU max abs error against float64 / e32: pyramid level 1 1.05e-7 / 1.05e-7; raw
patches 1.37e-6 / 1.37e-6, normalised 2.40e-5 / 2.72e-5; HardNet descriptors 1.17e-7 / 8.4e-8; AffNet and OriNet outputs 2.5e-8 /
4.2e-8 and 2.7e-8 / 5.1e-8, their LAF matrices 1.8e-6 / 1.3e-6 and 3.0e-6 / 9.0e-6; end to end LAFs 2.1e-5 / 2.9e-5, descriptors
1.12e-7 / 1.06e-7; 0 exemptions of 142 and 92 keypoints.  No stage needed the factor 4 (at most 1.4 e32).
"""
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import patchnet_ref as R  # noqa: E402

from openglue_amd import synthetic as syn  # noqa: E402
from openglue_amd.affnet_hardnet import AffNet, DoGAffNetHardNet, HardNet, OriNet, PatchPyramid, extract_patches  # noqa: E402
from openglue_amd.features import prepare_features_output  # noqa: E402
from openglue_amd.superglue import SuperGlue  # noqa: E402
from tests.util import parity_note  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
ULP = 2.0 ** -23
KINDS = {"hardnet": HardNet, "affnet": AffNet, "orinet": OriNet}


def _check(name, got, ref64, ref32):
    """GPU `got` against float64 under the tolerance rule; prints the figures before it asserts"""
    got = got.detach().cpu().double()
    assert got.shape == ref64.shape, (name, got.shape, ref64.shape)
    assert torch.isfinite(got).all(), name
    e32 = (ref32.double() - ref64).abs().max().item() if ref64.numel() else 0.0
    err = (got - ref64).abs().max().item() if ref64.numel() else 0.0
    floor = 4 * ULP * (ref64.abs().max().item() if ref64.numel() else 0.0)
    print(f"patchnet {name}: GPU max |d| {err:.3e}, e32 {e32:.3e}, bound {4 * e32 + floor:.3e}")
    assert err <= 4 * e32 + floor, (name, err, e32, floor)
    return err, e32


def _images(B, H, W, seed):
    return torch.cat([syn.make_image(H, W, seed=seed + i) for i in range(B)])


def _hand_lafs(B, H, W):
    """24 LAFs per image: scales 6, 11, 23 (level 0), 40, 55 (level 1), 80 (level 2, not built at 96 x 128); rotated, anisotropic;
    centres inside, within 3 px of each border, and one outside the image"""
    g = torch.Generator().manual_seed(11)
    out = torch.zeros(B, 24, 2, 3, dtype=torch.float64)
    edge = [(1.7, H / 2 + 0.3), (W - 2.4, H / 3), (W / 2 + 0.6, 2.2), (W / 3, H - 1.9), (W + 3.5, H / 2)]
    for b in range(B):
        i = 0
        for s in (6.0, 11.0, 23.0, 40.0, 55.0, 80.0):
            for v in range(4):
                th = float(torch.rand(1, generator=g)) * 6.283
                a = 1.0 if v == 0 else 1.0 + 1.5 * float(torch.rand(1, generator=g))
                sk = 0.0 if v < 2 else float(torch.rand(1, generator=g)) - 0.5
                c, sn = math.cos(th), math.sin(th)
                rotm = torch.tensor([[c, sn], [-sn, c]], dtype=torch.float64)
                shape = torch.tensor([[a, 0.0], [sk, 1.0 / a]], dtype=torch.float64)      # det 1
                out[b, i, :, :2] = s * (shape @ rotm)
                if (i + b) % 4 == 3:
                    x, y = edge[((i + b) // 4) % len(edge)]
                else:
                    x, y = float(torch.rand(1, generator=g)) * (W - 1), float(torch.rand(1, generator=g)) * (H - 1)
                out[b, i, 0, 2], out[b, i, 1, 2] = x, y
                i += 1
    return out


def test_pyramid_and_extract():
    B, H, W = 2, 96, 128
    img = _images(B, H, W, seed=20)
    lv64, lv32 = R.pyramid(img.double()), R.pyramid(img)
    assert [tuple(l.shape[-2:]) for l in lv64] == [(96, 128), (48, 64)]
    pyr = PatchPyramid(img.to(DEV))
    got = pyr.levels
    assert len(got) == 2
    for l in range(2):
        _check(f"pyramid level {l}", got[l], lv64[l], lv32[l])
    lafs = _hand_lafs(B, H, W)
    level, margin = R.level_of(lafs)
    assert margin.min().item() >= 0.05                                # no level decision is near a rounding: no exemptions
    assert sorted(set(level.flatten().tolist())) == [0, 1, 2]
    lafs32 = lafs.float()
    for upright in (False, True):
        p64, p32 = R.extract(lv64, lafs32.double(), upright), R.extract(lv32, lafs32, upright)
        raw = pyr.extract(lafs32.to(DEV), upright=upright)
        _check(f"extract upright={upright}", raw, p64, p32)
        assert torch.equal(raw.cpu()[level == 2], torch.zeros(int((level == 2).sum()), 1, 32, 32))
        nrm = pyr.extract(lafs32.to(DEV), upright=upright, normalize=True)
        _check(f"extract + normalise upright={upright}", nrm, R.normalize_patches(p64), R.normalize_patches(p32))
    assert torch.equal(extract_patches(img.to(DEV), lafs32.to(DEV)), pyr.extract(lafs32.to(DEV)))


def _net(kind, seed=2):
    net = KINDS[kind]()
    sd = syn.make_patchnet_state_dict(kind, seed=seed)
    net.load_state_dict(sd, strict=True)
    return net.eval().to(DEV), sd


@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("N", [1, 3, 65])
def test_each_net(kind, N):
    """N random patches of different content plus one constant patch (std 0): one patch, a partial tile, more than one workgroup"""
    net, sd = _net(kind)
    g = torch.Generator().manual_seed(100 + N)
    patches = torch.randn(N + 1, 1, 32, 32, generator=g) * (0.5 + torch.rand(N + 1, 1, 1, 1, generator=g)) + torch.randn(N + 1, 1, 1, 1, generator=g)
    patches[N] = 0.3
    r64, r32 = R.net_forward(sd, kind, patches.double()), R.net_forward(sd, kind, patches)
    out = net(patches.to(DEV))
    _check(f"{kind} n={N + 1}", out[:N], r64[:N], r32[:N])              # the constant patch apart: in fp32 on the CPU its mean is not
    _check(f"{kind} n={N + 1} constant patch", out[N:], r64[N:], r32[N:])   # exact and (x - mean) / 1e-6 is noise, which would widen e32
    one = net(patches[:1].to(DEV))                                    # a launch of a single patch gives the same row
    assert torch.equal(one[0], out[0])
    if kind == "hardnet":
        assert ((out.cpu().double().norm(dim=1) - 1).abs() < 1e-5).all()
        return
    lafs = torch.randn(N + 1, 2, 3, generator=g) * 8
    lafs[:, :, 2] = torch.rand(N + 1, 2, generator=g) * 90
    upd = R.affnet_update if kind == "affnet" else R.orinet_update
    l64, l32 = upd(lafs.double(), r64), upd(lafs, r32)
    dl = lafs.to(DEV).clone()
    net.run(patches.to(DEV), dl)
    _check(f"{kind} lafs n={N + 1}", dl[:N], l64[:N], l32[:N])
    _check(f"{kind} lafs n={N + 1} constant patch", dl[N:], l64[N:], l32[N:])
    assert torch.equal(dl.cpu()[:, :, 2], lafs[:, :, 2])


def _model(max_keypoints=128):
    m = DoGAffNetHardNet(max_keypoints=max_keypoints)
    sds = {k: syn.make_patchnet_state_dict(k, seed=3) for k in KINDS}
    m.hardnet.load_state_dict(sds["hardnet"], strict=True)
    m.affnet.load_state_dict(sds["affnet"], strict=True)
    m.orinet.angle_detector.load_state_dict(sds["orinet"], strict=True)
    return m.to(DEV), sds


@pytest.mark.parametrize("shape", [(2, 96, 128), (1, 120, 160)])
def test_end_to_end(shape):
    """the chain AffNet -> OriNet -> HardNet against the reference chain fed the LAFs of the GPU detector"""
    B, H, W = shape
    img = _images(B, H, W, seed=30)
    model, sds = _model()
    lafs0, scores0 = model.detect(img.to(DEV))
    lafs, scores, desc = model(img.to(DEV))
    n = lafs.shape[1]
    assert 16 <= n <= 128 and lafs.shape == (B, n, 2, 3) and scores.shape == (B, n) and desc.shape == (B, n, 128)
    assert torch.equal(scores, scores0) and torch.equal(lafs[..., 2], lafs0[..., 2])
    l64, d64, margin = R.chain(img.double(), lafs0.cpu().double(), sds)
    l32, d32, _ = R.chain(img, lafs0.cpu(), sds)
    keep = margin >= 1e-4
    exempt = int((~keep).sum())
    parity_note(f"patchnet end to end {shape}: exempt={exempt} of {B * n} keypoints")
    assert exempt <= max(1, 0.005 * B * n)
    _check(f"end to end {shape} lafs", lafs.cpu()[keep], l64[keep], l32[keep])
    _check(f"end to end {shape} descriptors", desc.cpu()[keep], d64[keep], d32[keep])
    # the LAFs now carry an affine shape: the scale is the detector's, the matrix is no similarity
    assert torch.allclose(R.scale_of(lafs.cpu().double()), R.scale_of(lafs0.cpu().double()), rtol=1e-5)
    A = lafs[..., :2].cpu()
    assert ((A[..., 0, 0] - A[..., 1, 1]).abs() + (A[..., 0, 1] + A[..., 1, 0]).abs()).max().item() > 1e-3


def test_determinism_and_wiring():
    img = _images(2, 96, 128, seed=30).to(DEV)
    model, _ = _model()
    a, b = model(img), model(img)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    one = model(img[:1])
    m = a[0].shape[1]
    assert 0 < m <= one[0].shape[1]
    for x, y in zip(a, one):                                          # min_stack keeps the strongest m of image 0, in the same order
        assert torch.equal(x[0], y[0, :m])
    empty = model(torch.full((1, 1, 64, 64), 0.5, device=DEV))
    assert empty[0].shape == (1, 0, 2, 3) and empty[1].shape == (1, 0) and empty[2].shape == (1, 0, 128)
    feats = prepare_features_output(*a, method="affine")
    side = feats["side_info"]
    assert side.shape == (2, m, 6) and torch.isfinite(side).all()
    cfg = syn.make_config(descriptor_dim=128, num_stages=2, num_heads=4, num_iters=3, side_info_size=6)
    sg = SuperGlue(cfg).eval()
    sg.load_state_dict(syn.make_state_dict(cfg, seed=0), strict=True)
    sg.to(DEV)
    data = {"keypoints0": feats["keypoints"][:1], "keypoints1": feats["keypoints"][1:], "local_descriptors0": feats["local_descriptors"][:1],
            "local_descriptors1": feats["local_descriptors"][1:], "side_info0": side[:1], "side_info1": side[1:],
            "image0_size": [128, 96], "image1_size": [128, 96]}
    out = sg.match(data, 0.2)
    torch.cuda.synchronize()
    sg.check_status()
    assert out["matches0"].shape == (1, m) and torch.isfinite(out["scores"]).all()
