"""The SuperPointNetBn fine-tuning kernels (csrc/superpoint_bn_train.hip) through the C ABI on integer-valued data at 3 x 24 x 1100: many
tiles per channel (619 flat tiles of 128 pixels at full resolution, the last one partial), partial tile columns, flat tiles that cross
images; NaN guard bands behind every buffer.

test_statistics_on_integers: og_superpoint_bn_train_forward with an integer image and integer conv1a weights.  The raw output of conv1a
    is then integer-valued and every pivoted partial sum (z - pivot, its square) is exact in fp32, so the float64 merge sees exact inputs:
    bn1a's saved mean and rstd, and its running buffers, equal the float64 values of the whole map rounded once to fp32, bit for bit.
    (The layers above see non-integer activations; tests/test_gpu_superpoint_bn_train.py holds them to the float64 oracle.)
test_reduction_partials_on_integers: og_superpoint_bn_train_backward with first_layer = 8 on a test-built saved buffer (integer raw map
    of the heads, integer means, scale 1) and an integer g_hidden: the per-tile (sum gy, sum gy (z - mean)) partials the reduction left
    in the workspace equal float64 bit for bit, d beta / d gamma equal the float64 sums, and dz (layer_grads) equals the formula.
Both assert the launched kernel instances by name.
"""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from openglue_amd import _lib, synthetic as syn
from openglue_amd.kernel_trace import launched_kernels, superpoint_bn_train_instances
from openglue_amd.superpoint import SuperPointNetBn, _BN_TRUNK, _GRAD_FLOATS

pytestmark = pytest.mark.gpu

B, H, W = 3, 24, 1100
GUARD = 1024
NAN = float("nan")
r64 = lambda n: (n + 63) // 64 * 64


def _dev():
    return torch.device("cuda:0")


def _saved_layout():
    """offsets (floats) as bn_saved_layout of the source: hidden, coef, z1a, z[0..7]"""
    dims = [(H, W, 64), (H // 2, W // 2, 64), (H // 2, W // 2, 64), (H // 4, W // 4, 128), (H // 4, W // 4, 128), (H // 8, W // 8, 128),
            (H // 8, W // 8, 128), (H // 8, W // 8, 512)]
    o, lay = 0, {}
    for name, n in [("hidden", B * (H // 8) * (W // 8) * 512), ("coef", 4 * 1280), ("z1a", B * H * W * 64)] + \
            [(f"z{j}", B * h * w * c) for j, (h, w, c) in enumerate(dims)]:
        lay[name] = (o, n)
        o += r64(n)
    return lay, o


def _buffers(fill_saved=NAN):
    lib = _lib.load()
    lay, total = _saved_layout()
    assert total * 4 == lib.og_superpoint_bn_train_saved_bytes(B, H, W)
    saved = torch.full((total + GUARD,), fill_saved, device=_dev())
    nws = lib.og_superpoint_bn_train_workspace_bytes(B, H, W)
    ws = torch.full((nws // 4 + GUARD,), NAN, device=_dev())
    assert saved.data_ptr() % 256 == 0 and ws.data_ptr() % 256 == 0
    return lay, total, saved, nws // 4, ws


def test_statistics_on_integers():
    dev = _dev()
    g = torch.Generator().manual_seed(0)
    net = SuperPointNetBn()
    net.load_state_dict(syn.make_superpoint_state_dict(True, seed=1))
    with torch.no_grad():
        net.conv1a.weight.copy_(torch.randint(-2, 3, (64, 1, 3, 3), generator=g).float())
        net.conv1a.bias.copy_(torch.randint(-3, 4, (64,), generator=g).float())
    net = net.to(dev)
    img = torch.randint(0, 4, (B, 1, H, W), generator=g).float()
    lay, total, saved, nws, ws = _buffers()
    mods = [getattr(net, n) for n in _BN_TRUNK]
    before = (net.bn1a.running_mean.clone().cpu().double(), net.bn1a.running_var.clone().cpu().double())
    bn = (C.c_void_p * 40)(*[t.data_ptr() for m in mods for t in (m.weight, m.bias, m.running_mean, m.running_var)])
    eps = (C.c_float * 10)(*[float(m.eps) for m in mods])
    mom = (C.c_float * 10)(*[float(m.momentum) for m in mods])
    gimg, packed = img.to(dev), net._pack_raw(dev)
    names = superpoint_bn_train_instances(launched_kernels(lambda: _lib.call(
        "og_superpoint_bn_train_forward", dev, B, H, W, gimg.data_ptr(), packed.data_ptr(), bn, eps, mom, saved.data_ptr(), ws.data_ptr(), _lib.STREAM)))
    conv = lambda bnw, inpool: f"sp_bn_conv3x3_kernel<{bnw},{inpool}>"
    want = ["sp_bn_conv1a_kernel"] + [conv(64, "false"), conv(64, "true"), conv(64, "false"), conv(128, "true"), conv(128, "false"),
                                      conv(128, "true"), conv(128, "false"), conv(128, "false")]
    got = [n.replace(" ", "") for n in names]
    assert [n for n in got if "conv" in n] == want, got
    assert got.count("sp_bn_stats_finish_kernel") == 9 and got[-1] == "sp_bn_act_kernel" and len(got) == 19
    assert bool(saved[total:].isnan().all()) and bool(ws[nws:].isnan().all())         # guard bands untouched
    for name, (o, n) in lay.items():
        assert not saved[o:o + n].isnan().any(), name                                 # every plane fully written
    o, n = lay["z1a"]
    z = saved[o:o + n].view(B, H, W, 64).cpu().double()
    ref = F.conv2d(img.double(), net.conv1a.weight.cpu().double(), net.conv1a.bias.cpu().double(), padding=1).permute(0, 2, 3, 1)
    assert torch.equal(z, ref)                                                       # integers: the raw output is exact
    N = B * H * W
    mean, var = z.reshape(N, 64).mean(0), z.reshape(N, 64).var(0, unbiased=False)
    coef = saved[lay["coef"][0]:lay["coef"][0] + 4 * 64].view(4, 64).cpu()
    f32 = lambda v: float(torch.tensor(v, dtype=torch.float32))                      # eps and momentum cross the ABI as fp32
    eps1a, m = f32(net.bn1a.eps), f32(net.bn1a.momentum)
    assert torch.equal(coef[0], mean.float()), (coef[0].double() - mean).abs().max()
    assert torch.equal(coef[1], torch.rsqrt(var + eps1a).float())
    assert torch.equal(coef[2], (net.bn1a.weight.cpu().double() * torch.rsqrt(var + eps1a)).float())
    assert torch.equal(coef[3], net.bn1a.bias.cpu())
    assert torch.equal(net.bn1a.running_mean.cpu(), ((1 - m) * before[0] + m * mean).float())
    assert torch.equal(net.bn1a.running_var.cpu(), ((1 - m) * before[1] + m * var * N / (N - 1)).float())


def test_reduction_partials_on_integers():
    dev = _dev()
    g = torch.Generator().manual_seed(1)
    Hc, Wc = H // 8, W // 8
    npix = B * Hc * Wc                                                                # 1233 = 9 flat tiles of 128 + 81: tiles cross the three images
    lay, total, saved, nws, ws = _buffers()
    z = torch.randint(-6, 7, (npix, 512), generator=g).float()
    mean = torch.randint(-2, 3, (512,), generator=g).float()
    rstd = torch.full((512,), 0.5)
    gamma = torch.randint(1, 3, (512,), generator=g).float() * torch.where(torch.rand(512, generator=g) < 0.3, -1.0, 1.0)   # some negative
    beta = torch.randint(-1, 2, (512,), generator=g).float()
    gh = torch.randint(-4, 5, (npix, 512), generator=g).float()
    o = lay["coef"][0] + 4 * 768                                                      # the heads are BatchNorm layer 8, channels 768..1279
    saved[o:o + 2048] = torch.cat([mean, rstd, gamma * rstd, beta]).to(dev)
    saved[lay["z7"][0]:lay["z7"][0] + npix * 512] = z.flatten().to(dev)
    # the weight gradient of the heads reads its input: the raw map of conv4b and its coefficients (BatchNorm layer 7)
    o7 = lay["coef"][0] + 4 * 640
    saved[o7:o7 + 512] = torch.cat([torch.zeros(128), torch.ones(128), torch.ones(128), torch.zeros(128)]).to(dev)
    saved[lay["z6"][0]:lay["z6"][0] + npix * 128] = torch.randint(-3, 4, (npix * 128,), generator=g).float().to(dev)
    grads = torch.full((_GRAD_FLOATS + GUARD,), NAN, device=dev)
    bng = torch.full((2 * 1280 + GUARD,), NAN, device=dev)
    dump_n = B * H * W * 64 * 2 + B * (H // 2) * (W // 2) * 64 * 2 + B * (H // 4) * (W // 4) * 128 * 2 + npix * 128 * 2 + npix * 512
    dump = torch.full((dump_n + GUARD,), NAN, device=dev)
    pg = torch.zeros(_lib.load().og_superpoint_train_packed_bytes(256) // 4, device=dev)     # not read: first_layer = 8 stops before the data gradient
    gimg, ggh = torch.zeros(B, 1, H, W, device=dev), gh.to(dev)
    names = superpoint_bn_train_instances(launched_kernels(lambda: _lib.call(
        "og_superpoint_bn_train_backward", dev, B, H, W, gimg.data_ptr(), pg.data_ptr(), saved.data_ptr(), ggh.data_ptr(), 8, grads.data_ptr(),
        bng.data_ptr(), dump.data_ptr(), ws.data_ptr(), _lib.STREAM)))
    got = [n.replace(" ", "") for n in names]
    assert got == ["sp_bn_reduce_kernel<false>", "sp_bn_reduce_finish_kernel", "sp_wgrad_kernel<SpBn,false,false>", "sp_reduce_parts_kernel",
                   "sp_grad_dump_kernel<SpBn,false>"], got
    assert bool(ws[nws:].isnan().all()) and bool(grads[_GRAD_FLOATS:].isnan().all()) and bool(bng[2560:].isnan().all()) and \
        bool(dump[dump_n:].isnan().all())
    # float64 restatement
    z64, g64, mu64 = z.double(), gh.double(), mean.double()
    y = (z64 - mu64) * (gamma * rstd).double() + beta.double()
    gy = torch.where(y > 0, g64, torch.zeros_like(g64))
    T = (npix + 127) // 128
    part = ws[:512 * T * 2].view(512, T, 2).cpu()                                     # the statistics / reduction partials open the workspace
    for t in range(T):
        rows = slice(128 * t, min(npix, 128 * t + 128))
        assert torch.equal(part[:, t, 0].double(), gy[rows].sum(0)), t                # bit for bit: every sum is an exact integer
        assert torch.equal(part[:, t, 1].double(), (gy[rows] * (z64[rows] - mu64)).sum(0)), t
    dbeta, dgamma = gy.sum(0), rstd.double() * (gy * (z64 - mu64)).sum(0)
    assert torch.equal(bng[768:1280].cpu(), dgamma.float()) and torch.equal(bng[1280 + 768:2560].cpu(), dbeta.float())
    assert bool(bng[:768].isnan().all()) and bool(bng[1280:1280 + 768].isnan().all())           # the layers below were not visited
    xhat = (z64 - mu64) * rstd.double()
    dz = (gamma * rstd).double() * (gy - dbeta / npix - xhat * dgamma / npix)
    got_dz = dump[dump_n - npix * 512:dump_n].view(npix, 512).cpu().double()
    assert float((got_dz - dz).abs().max()) <= 4e-7 * float(dz.abs().max())             # three fp32 roundings (k1, k2, the fmaf) of O(1) terms
    assert bool(dump[:dump_n - npix * 512].isnan().all())
