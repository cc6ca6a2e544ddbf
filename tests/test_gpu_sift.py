"""The SIFT extractor on the MI355X (openglue_amd/sift.py, csrc/sift.hip) against the float64 restatement (tests/sift_ref.py) and the
reference's own selection code (tests/golden/sift_select.npz).

Every stage is compared on identical inputs: the restatement is fed what the GPU fed its own next stage (its fp32 pyramid, its
keypoints), so that a difference is that stage's and discrete decisions are taken on the same numbers."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sift_ref as R  # noqa: E402

from openglue_amd import synthetic as syn  # noqa: E402
from openglue_amd.sift import SIFT, geometry, split_octaves  # noqa: E402
from tests.util import parity_note  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sift_select.npz")
SHAPES = {"64x64": (1, 64, 64, 500), "97x131": (1, 97, 131, 510), "3x120x160": (3, 120, 160, 520)}
MAX_DESCRIBED = 250          # keypoints per image the restatement describes (a Python loop)


def _images(B, H, W, seed):
    """synthetic.make_image quantised to 8 bits, [B, 1, H, W] float32"""
    return torch.cat([(syn.make_image(H, W, seed=seed + i) * 255).round() / 255 for i in range(B)]).to(torch.float32)


@functools.lru_cache(maxsize=None)
def _stages(shape, quantize=True):
    """every stage of one GPU run on SHAPES[shape], on the host"""
    B, H, W, seed = SHAPES[shape]
    net = SIFT(quantize=quantize)
    img = _images(B, H, W, seed)
    x = img.to(DEV)
    ws, counts = net.workspace(B, H, W, DEV), net.new_counts(B, DEV)
    gauss, dog = net.pyramid(x, ws)
    det_i, det_f = net.detect(dog, H, W, counts, ws)
    ori_i, ori_f = net.orient(gauss, H, W, det_i, det_f, counts, ws)
    raw = net.describe(gauss, H, W, ori_i, ori_f, counts, normalize=False)
    desc = net.describe(gauss, H, W, ori_i, ori_f, counts)
    torch.cuda.synchronize()
    geom = geometry(H, W)
    counts = counts.cpu().numpy()
    assert (counts[:B] <= geom.cap).all() and (counts[B:2 * B] <= geom.cap2).all(), counts
    return dict(img=img.numpy(), geom=geom, counts=counts, gauss=[g.cpu().numpy() for g in split_octaves(gauss, geom, 6)],
                dog=[d.cpu().numpy() for d in split_octaves(dog, geom, 5)], det_i=det_i.cpu().numpy(), det_f=det_f.cpu().numpy(),
                ori_i=ori_i.cpu().numpy(), ori_f=ori_f.cpu().numpy(), raw=raw.cpu().numpy(), desc=desc.cpu().numpy())


@pytest.mark.parametrize("shape", list(SHAPES))
def test_pyramid_and_dog(shape):
    """Each level against the restatement's blur of the level it was made from (the GPU's own fp32 image, or the exact upsampled
    8-bit image): bound 2 * taps * 2^-24 * 255, the fp32 accumulation bound over both passes (taps additions per pass, each rounding
    a partial sum of at most 255).  Decimation and the DoG subtraction are exact in fp32."""
    B, H, W, _ = SHAPES[shape]
    s = _stages(shape)
    sig = R.level_sigmas()
    assert s["geom"].octaves == R.octave_sizes(H, W)
    worst = chain = 0.0
    for b in range(B):
        g64, _ = R.pyramid(R.quantize(s["img"][b, 0]))
        for o, (h, w) in enumerate(s["geom"].octaves):
            g = s["gauss"][o][b]
            if o == 0:
                src0 = R.upsample2(R.quantize(s["img"][b, 0]))
            else:
                assert np.array_equal(g[0], s["gauss"][o - 1][b][R.S][0:2 * h:2, 0:2 * w:2]), (shape, b, o)
            for i in range(R.S + 3):
                if o > 0 and i == 0:
                    continue
                src = src0 if i == 0 else g[i - 1].astype(np.float64)
                bound = 2 * len(R.taps(sig[i])) * 2.0 ** -24 * 255
                err = float(np.abs(g[i] - R.blur(src, sig[i])).max())
                worst = max(worst, err / bound)
                assert err <= bound, (shape, b, o, i, err, bound)
                chain = max(chain, float(np.abs(g[i] - g64[o][i]).max()))
            assert np.array_equal(s["dog"][o][b], g[1:] - g[:-1]), (shape, b, o)
    parity_note(f"sift pyramid {shape}: worst level error {worst:.3f} of its bound; against the full float64 chain max |d| {chain:.3e}")


@pytest.mark.parametrize("shape", list(SHAPES))
def test_detect(shape):
    """The restatement on the GPU's own fp32 DoG volume: identical candidates, fp64 outputs within 1e-9 relative."""
    B = SHAPES[shape][0]
    s = _stages(shape)
    total = 0
    for b in range(B):
        ki, kf = R.detect([d[b] for d in s["dog"]])
        n = int(s["counts"][b])
        assert n == len(ki), (shape, b, n, len(ki))
        assert np.array_equal(s["det_i"][b, :n], ki), (shape, b)
        rel = np.abs(s["det_f"][b, :n] - kf) / np.abs(kf)
        assert rel.max() <= 1e-9, (shape, b, rel.max())
        total += n
    assert total > 10
    print(f"sift detect {shape}: {total} keypoints")


@pytest.mark.parametrize("shape", list(SHAPES))
def test_orient(shape):
    """Fed the GPU's keypoints: one keypoint per histogram peak, the same peaks in the same order; a keypoint whose peak decision lies
    within 1e-4 (relative to the maximum) of the 0.8 line is exempt, at most 1 % of them.  Angles within 1e-3 degrees."""
    B = SHAPES[shape][0]
    s = _stages(shape)
    exempt = total = 0
    for b in range(B):
        n, n2 = int(s["counts"][b]), int(s["counts"][B + b])
        gauss = [g[b].astype(np.float64) for g in s["gauss"]]
        oi, of, near = R.orient(gauss, s["det_i"][b, :n].astype(np.int64), s["det_f"][b, :n])
        gi, gf = s["ori_i"][b, :n2], s["ori_f"][b, :n2]
        assert (np.diff(gi[:, 5]) >= 0).all()
        total += n
        for k in range(n):
            mine, ref = np.nonzero(gi[:, 5] == k)[0], np.nonzero(oi[:, 5] == k)[0]
            same = len(mine) == len(ref) and np.array_equal(gi[mine, :5], oi[ref, :5])
            if same:
                dang = np.abs((gf[mine, 3].astype(np.float64) - of[ref, 3] + 180.0) % 360.0 - 180.0)
                same = bool((dang <= 1e-3).all()) and np.array_equal(gf[mine][:, [0, 1, 2, 4]], of[ref][:, [0, 1, 2, 4]])
            if not same:
                assert near[k] < 1e-4, (shape, b, k, near[k], gf[mine], of[ref])
                exempt += 1
    parity_note(f"sift orient {shape}: exempt={exempt} of {total} keypoints")
    assert exempt <= 0.01 * total


@pytest.mark.parametrize("shape", list(SHAPES))
def test_describe(shape):
    """Fed the GPU's oriented keypoints and its fp32 Gaussian images: float descriptors within 1e-4; OpenCV's bytes differ by at most
    1 in at most 0.5 % of the elements."""
    B = SHAPES[shape][0]
    sq, sf = _stages(shape), _stages(shape, quantize=False)
    worst = 0.0
    off = elems = 0
    for b in range(B):
        n2 = int(sq["counts"][B + b])
        rows = np.arange(0, n2, max(1, n2 // MAX_DESCRIBED))
        gauss = [g[b].astype(np.float64) for g in sq["gauss"]]
        oi, of = sq["ori_i"][b, rows].astype(np.int64), sq["ori_f"][b, rows]
        assert np.array_equal(sf["ori_f"][b, rows], of)
        ref = R.describe(gauss, oi, of, quantize=False, rootsift=True)
        worst = max(worst, float(np.abs(sf["desc"][b, rows] - ref).max()))
        raw = np.stack([R.finish_descriptor(R.raw_descriptor(gauss, oi[k], of[k, 2], of[k, 3]), True) for k in range(len(rows))])
        d = np.abs(sq["raw"][b, rows] - raw)
        assert d.max() <= 1, (shape, b, d.max())
        off += int((d > 0).sum())
        elems += d.size
        refq = R.normalize_descriptors(sq["raw"][b, rows], True)           # the final step on the GPU's own bytes
        assert np.abs(sq["desc"][b, rows] - refq).max() <= 1e-6
    parity_note(f"sift describe {shape}: float descriptors max |d| {worst:.3e}; bytes off by one in {off} of {elems} elements")
    assert worst <= 1e-4
    assert off <= 0.005 * elems


def _select_on_gpu(of, desc, diameter, max_kpts, H=120, W=160, keys=None):
    """og_sift_select + og_sift_gather on given keypoints of one image -> (sel indices, lafs, scores, descriptors)"""
    n = len(of)
    net, geom = SIFT(max_keypoints=max_kpts, nms_diameter=diameter), geometry(H, W)
    assert n <= geom.cap2
    ori_i = torch.zeros(1, geom.cap2, 6, dtype=torch.int32)
    if keys is not None:
        ori_i[0, :n, :5] = torch.from_numpy(np.asarray(keys, dtype=np.int32))
    ori_f = torch.zeros(1, geom.cap2, 5, dtype=torch.float32)
    ori_f[0, :n] = torch.from_numpy(np.asarray(of, dtype=np.float32))
    d = torch.zeros(1, geom.cap2, 128, dtype=torch.float32)
    d[0, :n] = torch.from_numpy(np.asarray(desc, dtype=np.float32))
    counts = torch.zeros(5, dtype=torch.int32)
    counts[1] = n
    ori_i, ori_f, d, counts = ori_i.to(DEV), ori_f.to(DEV), d.to(DEV), counts.to(DEV)
    ws = net.workspace(1, H, W, DEV)
    sel = net.select(H, W, ori_i, ori_f, counts, ws)
    m = net.check_counts(counts.cpu(), 1, geom)
    lafs, scores, descs = net.gather(H, W, m, sel, ori_f, d)
    torch.cuda.synchronize()
    return sel[0, :m].cpu().numpy().astype(np.int64), lafs[0].cpu().numpy(), scores[0].cpu().numpy(), descs[0].cpu().numpy()


def test_select_equals_the_reference():
    """og_sift_select against the reference's detect_kpts_opencv run on the same seeded keypoints (n = 1, 7, 600, 6000; radius 4.5 and
    none; max_keypoints -1, 512, > n): the kept keypoints and their order are exact.  LAF entries: the angle is a float32 of up to
    2 pi, one rounding of it moves an entry by scale * 2^-22, so 4 such steps are allowed; centres, scores and descriptors are copies."""
    z = np.load(GOLDEN)
    ls, ds = int(z["row_stride"]), int(z["desc_stride"])
    for n in (int(v) for v in z["sizes"]):
        of, desc = R.synthetic_keypoints(n, seed=n)
        for di, d in enumerate(z["diameters"]):
            for mk in (-1, 512, n + 10):
                for rs in (1, 0):
                    name = f"n{n}_d{di}_k{mk}_r{rs}"
                    nd = R.normalize_descriptors(desc, bool(rs)).astype(np.float32)
                    sel, lafs, scores, descs = _select_on_gpu(of, nd, float(d), mk)
                    keep = z[name + "_keep"].astype(np.int64)
                    assert np.array_equal(sel, keep), name
                    assert np.array_equal(scores, of[keep, 4]), name
                    ref = z[name + "_lafs"]
                    tol = 6.0 * of[keep[::ls], 2].astype(np.float64)[:, None, None] * 2.0 ** -20 + 1e-6 * np.abs(ref)
                    assert (np.abs(lafs[::ls] - ref) <= tol).all(), name
                    assert np.array_equal(lafs[:, :, 2], of[keep, :2]), name
                    assert np.abs(descs[::ds] - z[name + "_desc"]).max() <= 1e-6, name


def test_select_chain_and_ties():
    """every point suppresses the next (the parallel rounds need as many sweeps as the chain is long), and equal responses ordered by key"""
    n = 53
    of = np.zeros((2 * n, 5), dtype=np.float32)
    of[:n, 0], of[:n, 1] = np.arange(n) * 3.0, 10.0
    of[n:, 0], of[n:, 1] = np.arange(n) * 3.0, 60.0
    of[:, 2] = 4.0
    of[:n, 4] = np.linspace(1.0, 0.5, n)
    of[n:, 4] = np.linspace(0.2, 0.45, n)              # the second chain runs the other way
    desc = np.zeros((2 * n, 128), dtype=np.float32)
    sel, _, _, _ = _select_on_gpu(of, desc, 9.0, -1)
    ref = R.select(of[:, :2], of[:, 4], np.arange(2 * n), 9.0, -1)
    assert np.array_equal(sel, ref) and len(sel) == 2 * ((n + 1) // 2)
    # ties: the same response everywhere, no NMS: the order is the key's, then the index
    of[:, 4] = 0.25
    keys = np.zeros((2 * n, 5), dtype=np.int64)
    keys[:, 0] = np.arange(2 * n)[::-1] % 3
    keys[:, 3] = (np.arange(2 * n) * 7) % 11
    sel, _, _, _ = _select_on_gpu(of, desc, -1.0, 40, keys=keys)
    ref = R.select(of[:, :2], of[:, 4], R.sort_keys(keys), -1.0, 40)
    assert np.array_equal(sel, ref)


def _run(net, img):
    out = net(img.to(DEV))
    torch.cuda.synchronize()
    return out


def test_module_outputs():
    B, H, W, seed = SHAPES["3x120x160"]
    img = _images(B, H, W, seed)
    net = SIFT()
    lafs, scores, desc = _run(net, img)
    n = scores.shape[1]
    assert n > 20 and lafs.shape == (B, n, 2, 3) and desc.shape == (B, n, 128)
    assert lafs.dtype == scores.dtype == desc.dtype == torch.float32 and lafs.is_cuda
    assert bool((scores[:, 1:] <= scores[:, :-1]).all())
    assert torch.isfinite(desc).all() and torch.isfinite(lafs).all()
    assert (desc.pow(2).sum(-1) - 1).abs().max() < 1e-5              # RootSIFT rows have unit L2 norm
    again = _run(net, img)
    for a, b in zip((lafs, scores, desc), again):
        assert torch.equal(a, b)
    singles = [_run(net, img[b:b + 1]) for b in range(B)]
    assert len({s[1].shape[1] for s in singles}) > 1 and n == min(s[1].shape[1] for s in singles)      # min_stack engaged
    for b in range(B):
        for a, s in zip((lafs, scores, desc), singles[b]):
            assert torch.equal(a[b], s[0, :n])
    # against the restatement of the whole extractor: the same keypoints in the same order (image 0)
    rl, rs, rd, _, _ = R.extract(img[0, 0].numpy())
    m = min(n, len(rs))
    same = np.abs(singles[0][0][0, :m, :, 2].cpu().numpy() - rl[:m, :, 2]).max(axis=1) < 1e-3
    print(f"sift module: {int(same.sum())} of {m} keypoints at the restatement's positions in its order")
    up = _run(SIFT(upright=True), img[:1])
    assert up[1].shape[1] > 20 and bool((up[0][0, :, 0, 1] == 0).all()) and bool((up[0][0, :, 0, 0] > 0).all())


def test_module_max_keypoints_and_empty():
    img = _images(1, 97, 131, 510)
    full = _run(SIFT(), img)
    n = full[1].shape[1]
    for k in (n - 7, n, n + 7):
        out = _run(SIFT(max_keypoints=k), img)
        m = min(k, n)
        assert out[1].shape == (1, m)
        for a, b in zip(out, full):
            assert torch.equal(a[0], b[0, :m])
    lafs, scores, desc = _run(SIFT(), torch.full((2, 1, 64, 80), 0.5))
    assert lafs.shape == (2, 0, 2, 3) and scores.shape == (2, 0) and desc.shape == (2, 0, 128)


def _pair_share(kp0, d0, kp1, d1, Hm):
    """share of mutual nearest-neighbour descriptor matches that land within 3 px of the ground truth"""
    dist = ((d0[:, None, :] - d1[None, :, :]) ** 2).sum(-1)
    a, b = dist.argmin(1), dist.argmin(0)
    i = np.nonzero(b[a] == np.arange(len(a)))[0]
    p = np.concatenate([kp0[i], np.ones((len(i), 1))], axis=1) @ Hm.T
    err = np.hypot(p[:, 0] / p[:, 2] - kp1[a[i], 0], p[:, 1] / p[:, 2] - kp1[a[i], 1])
    return float((err <= 3.0).mean()), len(i)


def test_homography_pair():
    """The bar is the restatement's own share on the same pair minus 2 percentage points for fp32."""
    H, W = 240, 320
    img0 = syn.make_image(H, W, seed=41)
    Hm = syn.random_homography(H, W, seed=42)
    img1 = syn.warp_image(img0, Hm)
    pair = [((im * 255).round() / 255).to(torch.float32) for im in (img0, img1)]
    net = SIFT(max_keypoints=512)
    gpu, ref = [], []
    for im in pair:
        lafs, _, desc = _run(net, im)
        gpu.append((lafs[0, :, :, 2].cpu().numpy().astype(np.float64), desc[0].cpu().numpy().astype(np.float64)))
        rl, _, rd, _, _ = R.extract(im[0, 0].numpy(), max_keypoints=512)
        ref.append((rl[:, :, 2], rd))
    share_gpu, n_gpu = _pair_share(*gpu[0], *gpu[1], Hm.numpy())
    share_ref, n_ref = _pair_share(*ref[0], *ref[1], Hm.numpy())
    parity_note(f"sift homography pair 240x320: {share_gpu:.3f} of {n_gpu} mutual matches within 3 px on the GPU, "
                f"{share_ref:.3f} of {n_ref} in float64")
    assert n_gpu >= 50
    assert share_gpu >= share_ref - 0.02


def test_through_the_matcher():
    from examples.openglue_matcher import OpenGlueMatcher
    from openglue_amd.superglue import SuperGlue
    H, W = 240, 320
    img0 = syn.make_image(H, W, seed=41)
    img1 = syn.warp_image(img0, syn.random_homography(H, W, seed=42))
    cfg = syn.make_config(descriptor_dim=128, num_stages=2, num_heads=4, num_iters=20, side_info_size=1)
    sg = SuperGlue(cfg).eval()
    sg.load_state_dict(syn.make_state_dict(cfg, seed=0), strict=True)
    sg.to(DEV)
    matcher = OpenGlueMatcher(SIFT(max_keypoints=512), sg, {"superglue": {"laf_to_sideinfo_method": "none"}, "inference": {"match_threshold": 0.0}})
    out = matcher({"image0": img0.to(DEV), "image1": img1.to(DEV)})
    torch.cuda.synchronize()
    n = out["keypoints0"].shape[0]
    assert out["keypoints0"].shape == out["keypoints1"].shape == (n, 2) and out["confidence"].shape == (n,)
    for v in out.values():
        if v.is_floating_point():
            assert torch.isfinite(v).all()
    print(f"sift through the matcher: {n} matches")
