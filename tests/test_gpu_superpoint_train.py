"""Fine-tuning SuperPointNet on the GPU: the gradients of openglue_amd.superpoint.SuperPointNet in train() mode against float64 torch
autograd of tests/superpoint_ref.py (dense + describe) on the CPU.

Discrete decisions are kept out of the comparison: the keypoints are those of the GPU forward (lafs[..., 2]); the oracle evaluates its
float64 heatmap and describe() at those pixels.  Loss = sum(scores * Gs) + sum(descriptors * Gd) with seeded normal cotangents.
Per parameter tensor err = max|g_gpu - g_64| / max|g_64|; the yardstick is fp32 ATen autograd on the CPU for the same loss, computed
alongside, and the bar is err <= FACTOR x (ATen-fp32 err of that tensor).

Measured on an MI355X (every parity test prints its figures before it asserts; DESIGN.md 4.8b has the table), err per tensor and, in
brackets, its ratio to the ATen-fp32 error:
    b2_44x60         trunk + detector head 2.1e-6 .. 5.0e-6 (1.1 .. 3.4)   descriptor head 3.0e-7 .. 5.9e-7 (0.8 .. 1.8)   worst convPb.weight 3.43
    b1_72x136        trunk + detector head 1.5e-6 .. 2.8e-6 (1.1 .. 3.2)   descriptor head 2.3e-7 .. 6.6e-7 (1.0 .. 1.1)   worst convPb.weight 3.21
    b1_8x8           trunk + detector head 6.2e-8 .. 9.0e-7 (0.6 .. 2.7)   descriptor head 1.5e-7 .. 7.3e-7 (1.1 .. 1.3)   worst conv1a.bias   2.73
    b2_44x60_top16   trunk + detector head 1.2e-6 .. 3.5e-6 (0.7 .. 1.4)   descriptor head 2.1e-7 .. 5.7e-7 (0.6 .. 2.2)   worst convDb.weight 2.21
    chain            trunk + detector head 2.6e-6 .. 5.0e-6 (0.9 .. 2.1)   descriptor head 3.3e-7 .. 1.2e-6 (0.6 .. 2.3)   worst convDb.weight 2.32
(with the data gradient summed per pass of 32 channels, tests/test_gpu_superpoint_train_forms.py; one chain over 9 Cin products gave 3.97 at b1_8x8).
They do not sit well below the bar, so FACTOR stays 4.  The factor does not cover a max-pool decision that falls differently in the fp32
forward (pinned bit for bit to the inference kernels) and in float64: an earlier version of the chain case, built from a 72 x 144 image,
had one conv1b window whose two largest float64 activations differ by 4.8e-7 relative; fp32 picked the other pixel, and conv1b.weight /
conv1a.weight came out 3.0e-4 / 1.3e-4 off (36x / 26x ATen, every other tensor within the bar).  The chain case now uses the image of
b1_72x136 itself, as the case is specified.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

import superpoint_ref as R
from openglue_amd import features, synthetic as syn
from openglue_amd.superpoint import CONV_NAMES, SuperPointNet

pytestmark = pytest.mark.gpu

FACTOR = 4.0            # the bar of the issue: a different summation order over up to B*H*W pixels, and a pool / ReLU decision that differs
                        # between fp32 and fp64 moves a whole gradient element

CASES = {
    "b2_44x60": dict(B=2, H=44, W=60, kw={}),                                         # no multiple of 8 or of the 8 x 16 tile; the third pool drops a row and a column; 22 / 21 candidates: min_stack cuts
    "b1_72x136": dict(B=1, H=72, W=136, kw={}),                                       # nine tile rows, a half tile column
    "b1_8x8": dict(B=1, H=8, W=8, kw=dict(remove_borders_size=0, nms_kernel=3)),      # one cell, one tile
    "b2_44x60_top16": dict(B=2, H=44, W=60, kw=dict(max_keypoints=16)),               # top-k cuts: the gathered order is by score
}


def _dev():
    return torch.device("cuda:0")


def _net(**kw):
    net = SuperPointNet(**kw)
    net.load_state_dict(syn.make_superpoint_state_dict(False, seed=1))
    return net.to(_dev())


def _images(B, H, W):
    return torch.cat([syn.make_image(H, W, seed=5 + i) for i in range(B)])


def _describe(desc_nhwc, xy, dtype):
    """superpoint_ref.describe in `dtype` (that one always computes in float64)"""
    Hc, Wc, D = desc_nhwc.shape
    p = (xy.to(dtype) - 4 + 0.5) / torch.tensor([Wc * 8 - 4.5, Hc * 8 - 4.5], dtype=dtype) * 2 - 1
    d = F.grid_sample(desc_nhwc.permute(2, 0, 1)[None], p.view(1, 1, -1, 2), mode="bilinear", align_corners=False)
    return F.normalize(d.view(D, -1).t(), p=2, dim=1)


def _oracle_grads(img, xy, Gs, Gd, dtype):
    """torch autograd on the CPU in `dtype`: {state-dict key: gradient} of sum(scores * Gs) + sum(descriptors * Gd) at the pixels xy"""
    sd = {k: v.detach().clone().to(dtype).requires_grad_(True) for k, v in syn.make_superpoint_state_dict(False, seed=1).items()}
    heat, desc = R.dense(sd, img, dtype=dtype)
    loss = 0
    for b in range(img.shape[0]):
        x, y = xy[b, :, 0].long(), xy[b, :, 1].long()
        loss = loss + (heat[b, y, x] * Gs[b].to(dtype)).sum() + (_describe(desc[b], xy[b], dtype) * Gd[b].to(dtype)).sum()
    loss.backward()
    return {k: v.grad for k, v in sd.items()}


def _gpu_grads(net):
    return {f"{n}.{k}": getattr(getattr(net, n), k).grad for n in CONV_NAMES for k in ("weight", "bias")}


def _cotangents(B, n, seed=3):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, n, generator=g, dtype=torch.float64), torch.randn(B, n, 256, generator=g, dtype=torch.float64)


@functools.lru_cache(maxsize=None)
def _run(case):
    """One train-mode forward + backward of a case, shared (and left unchanged) by the tests that need it."""
    c = CASES[case]
    img = _images(c["B"], c["H"], c["W"])
    net = _net(**c["kw"]).train()
    lafs, scores, desc = net(img.to(_dev()))
    n = scores.shape[1]
    Gs, Gd = _cotangents(c["B"], n)
    (scores * Gs.to(_dev(), torch.float32)).sum().add((desc * Gd.to(_dev(), torch.float32)).sum()).backward()
    torch.cuda.synchronize()
    return dict(net=net, img=img, lafs=lafs.detach(), scores=scores.detach(), desc=desc.detach(), Gs=Gs, Gd=Gd, grads=_gpu_grads(net))


def _compare(name, gpu, g64, g32):
    """prints every tensor's figures, then asserts the bar"""
    bad = []
    for k in g64:
        den = g64[k].abs().max().item()
        e_gpu = (gpu[k].detach().cpu().double() - g64[k]).abs().max().item() / den
        e_aten = (g32[k].double() - g64[k]).abs().max().item() / den
        print(f"{name} {k:14s} max|g| {den:.3e}  gpu {e_gpu:.2e}  aten-fp32 {e_aten:.2e}  ratio {e_gpu / max(e_aten, 1e-30):.2f}")
        if not e_gpu <= FACTOR * e_aten:
            bad.append((k, e_gpu, e_aten))
    assert not bad, f"{name}: gradient error above {FACTOR} x ATen-fp32: {bad}"


@pytest.mark.parametrize("case", list(CASES))
def test_gradient_parity(case):
    r = _run(case)
    n = r["scores"].shape[1]
    assert n >= (4 if case == "b1_8x8" else 8), f"{n} keypoints"
    assert r["scores"].shape == (CASES[case]["B"], n) and r["desc"].shape == (CASES[case]["B"], n, 256)
    xy = r["lafs"][..., 2].cpu()
    g64 = _oracle_grads(r["img"], xy, r["Gs"], r["Gd"], torch.float64)
    g32 = _oracle_grads(r["img"], xy, r["Gs"], r["Gd"], torch.float32)
    _compare(case, r["grads"], g64, g32)


def test_selection_is_cut_by_score():
    """the cases above do exercise min_stack / top-k: unequal candidate counts, outputs in descending score"""
    r = _run("b2_44x60_top16")
    net, img = r["net"], r["img"].to(_dev())
    with torch.no_grad():
        B, _, H, W = img.shape
        ws = net._workspace(B, H, W, img.device)
        counts = net.detect(net.dense(img, ws)[0], ws)[0].cpu()
    assert counts[0] != counts[1] and int(counts[:2].min()) > 16 and r["scores"].shape[1] == 16
    assert bool((r["scores"][:, 1:] <= r["scores"][:, :-1]).all())
    assert _run("b2_44x60")["scores"].shape[1] == int(counts[:2].min())               # min_stack cut the larger image


@pytest.mark.parametrize("case", list(CASES))
def test_forward_identity(case):
    """train() with grad enabled returns the eval() tensors bit for bit, with a grad_fn on scores and descriptors only"""
    c = CASES[case]
    img = _images(c["B"], c["H"], c["W"]).to(_dev())
    net = _net(**c["kw"])
    ref = net.eval()(img)
    assert all(t.grad_fn is None and not t.requires_grad for t in ref)
    out = net.train()(img)
    assert out[0].grad_fn is None and not out[0].requires_grad
    assert out[1].grad_fn is not None and out[2].grad_fn is not None
    for a, b in zip(ref, out):
        assert torch.equal(a, b.detach())
    with torch.no_grad():                            # grad disabled: today's path even in train()
        quiet = net(img)
    assert all(t.grad_fn is None for t in quiet) and all(torch.equal(a, b) for a, b in zip(ref, quiet))


def test_determinism():
    """two forward + backward runs: bit-identical gradients for every parameter"""
    first = _run("b2_44x60")
    c = CASES["b2_44x60"]
    net = _net(**c["kw"]).train()
    lafs, scores, desc = net(first["img"].to(_dev()))
    (scores * first["Gs"].to(_dev(), torch.float32)).sum().add((desc * first["Gd"].to(_dev(), torch.float32)).sum()).backward()
    for k, g in _gpu_grads(net).items():
        assert g is not None and torch.equal(g, first["grads"][k]), k


def test_dropped_pixel_gradient():
    """44 x 60: the 11 x 15 level loses its last row and column in the third pool; the gradient that reaches them is exactly 0, and the
    gradient of the kept pixels is not"""
    c = CASES["b2_44x60"]
    net = _net(**c["kw"]).train()
    net.keep_layer_grads = True
    lafs, scores, desc = net(_images(c["B"], c["H"], c["W"]).to(_dev()))
    (scores.sum() + desc.sum()).backward()
    g = net.layer_grads["conv3b"]                    # gradient of conv3b's pre-activation output, [B, 11, 15, 128]
    assert g.shape == (2, 11, 15, 128)
    assert float(g[:, 10].abs().max()) == 0.0 and float(g[:, :, 14].abs().max()) == 0.0
    assert float(g[:, :10, :14].abs().max()) > 0.0
    g1 = net.layer_grads["conv1b"]                   # 44 x 60 -> 22 x 30: nothing dropped, every window routes to exactly one pixel
    assert g1.shape == (2, 44, 60, 64)
    nz = (g1.view(2, 22, 2, 30, 2, 64) != 0).sum(dim=(2, 4))
    assert int(nz.max()) <= 1


def test_no_keypoints():
    net = _net(keypoint_threshold=2.0).train()
    lafs, scores, desc = net(_images(2, 44, 60).to(_dev()))
    assert lafs.shape == (2, 0, 2, 3) and scores.shape == (2, 0) and desc.shape == (2, 0, 256)
    (scores.sum() + desc.sum()).backward()
    for p in net.parameters():
        assert p.grad is not None and p.grad.shape == p.shape and not p.grad.any()


def test_requires_grad_on_convDb_only():
    r = _run("b2_44x60")
    net = _net().train()
    for name, p in net.named_parameters():
        p.requires_grad_(name.startswith("convDb"))
    lafs, scores, desc = net(r["img"].to(_dev()))
    (scores * r["Gs"].to(_dev(), torch.float32)).sum().add((desc * r["Gd"].to(_dev(), torch.float32)).sum()).backward()
    for name, p in net.named_parameters():
        if name.startswith("convDb"):
            assert torch.equal(p.grad, r["grads"][name]), name
        else:
            assert p.grad is None, name


def test_non_contiguous_cotangent():
    r = _run("b2_44x60")
    net = _net().train()
    lafs, scores, desc = net(r["img"].to(_dev()))
    B, n = scores.shape
    Gd = torch.empty(B, 256, n, device=_dev()).copy_(r["Gd"].to(_dev(), torch.float32).transpose(1, 2)).transpose(1, 2)
    Gs = torch.empty(n, B, device=_dev()).copy_(r["Gs"].to(_dev(), torch.float32).t()).t()
    assert not Gd.is_contiguous() and not Gs.is_contiguous()
    torch.autograd.backward([scores, desc], [Gs, Gd])
    for k, g in _gpu_grads(net).items():
        assert torch.equal(g, r["grads"][k]), k


@pytest.mark.parametrize("log_response", [False, True])
def test_response_path(log_response):
    g = torch.Generator().manual_seed(0)
    B, N = 2, 37
    lafs = torch.zeros(B, N, 2, 3)
    lafs[..., 0, 0] = lafs[..., 1, 1] = 1.0 + torch.rand(B, N, generator=g)
    lafs[..., 2] = 50.0 * torch.rand(B, N, 2, generator=g)
    resp = torch.rand(B, N, generator=g)
    desc = torch.randn(B, N, 8, generator=g)
    lafs, resp, desc = lafs.to(_dev()), resp.to(_dev()), desc.to(_dev())
    plain = features.prepare_features_output(lafs, resp, desc, "scale", log_response=log_response)
    assert plain["side_info"].grad_fn is None and plain["keypoints"].grad_fn is None
    r = resp.clone().requires_grad_(True)
    out = features.prepare_features_output(lafs, r, desc, "scale", log_response=log_response)
    assert out["side_info"].grad_fn is not None and out["keypoints"].grad_fn is None
    assert torch.equal(out["side_info"].detach(), plain["side_info"]) and torch.equal(out["keypoints"], plain["keypoints"])
    G = torch.randn(B, N, 2, generator=g).to(_dev())
    (out["side_info"] * G).sum().backward()
    r2 = resp.clone().requires_grad_(True)
    ((torch.log(r2 + 0.1) if log_response else r2) * G[..., 0]).sum().backward()
    assert torch.allclose(r.grad, r2.grad, rtol=1e-6, atol=0)
    with torch.no_grad():                            # grad disabled: today's call, whatever the flag on the input
        quiet = features.prepare_features_output(lafs, r, desc, "scale", log_response=log_response)
    assert quiet["side_info"].grad_fn is None and torch.equal(quiet["side_info"], plain["side_info"])


def test_chain_through_superglue():
    """extractor -> prepare_features_output -> SuperGlue.train() -> loss: the gradients the matcher hands back, fed to the float64
    oracle as Gs / Gd, reproduce the extractor's parameter gradients under the same rule"""
    from openglue_amd.superglue import SuperGlue
    H, W = 72, 136
    base = _images(1, H, W)                                                           # the image of the b1_72x136 case
    img = torch.cat([base, torch.roll(base, -8, dims=3)])                             # image 0, and image 1 = its crop shifted by 8 pixels (the 8 columns that leave re-enter on the right)
    net = _net(max_keypoints=48).train()
    lafs, scores, desc = net(img.to(_dev()))
    scores.retain_grad()
    desc.retain_grad()
    n = scores.shape[1]
    assert n == 48
    f0 = features.prepare_features_output(lafs[:1], scores[:1], desc[:1], "none")
    f1 = features.prepare_features_output(lafs[1:], scores[1:], desc[1:], "none")
    cfg = syn.make_config(descriptor_dim=256, num_stages=2, num_heads=4, num_iters=20, side_info_size=1)
    model = SuperGlue(cfg)
    model.load_state_dict(syn.make_state_dict(cfg, seed=0))
    model = model.to(_dev()).train()
    data = {"image0_size": [W, H], "image1_size": [W, H]}
    for i, f in enumerate((f0, f1)):
        data.update({f"keypoints{i}": f["keypoints"], f"side_info{i}": f["side_info"], f"local_descriptors{i}": f["local_descriptors"]})
    y = model(data)
    loss = -y["scores"][:, :n, :n].diagonal(dim1=1, dim2=2).mean()
    loss.backward()
    assert scores.grad is not None and desc.grad is not None and float(desc.grad.abs().max()) > 0 and float(scores.grad.abs().max()) > 0
    xy = lafs[..., 2].detach().cpu()
    Gs, Gd = scores.grad.cpu().double(), desc.grad.cpu().double()
    g64 = _oracle_grads(img, xy, Gs, Gd, torch.float64)
    g32 = _oracle_grads(img, xy, Gs, Gd, torch.float32)
    _compare("chain", _gpu_grads(net), g64, g32)
