"""Fine-tuning SuperPointNetBn on the GPU: openglue_amd.superpoint.SuperPointNetBn in train() mode (batch statistics in every BatchNorm,
csrc/superpoint_bn_train.hip) against the float64 oracle of tests/superpoint_bn_ref.py on the CPU.

Discrete decisions are kept out of the comparison as in tests/test_gpu_superpoint_train.py: the keypoints are those of the GPU forward;
the oracle evaluates its float64 heatmap and describe() at those pixels, and the inputs have no pool window closer than 1e-5 relative
(tests/test_superpoint_bn_train_cpu.py).  Per tensor err = max|gpu - f64| / max|f64|; the yardstick is fp32 ATen on the CPU computed
alongside, the bar err <= FACTOR x (ATen-fp32 err of that tensor), FACTOR = 4 as in tests/test_gpu_superpoint_train.py.  Every parity
test prints its figures before it asserts.

Measured on an MI355X, worst ratio to the ATen-fp32 error over the tensors of a case, forward (scores, descriptors, the 24 running
buffers after one and two steps) / gradients (36 tensors):
    b2_44x60    1.95 (bn4b.running_mean, 2.1e-7)   / 2.16 (conv4a.weight, 2.5e-6)
    b1_72x136   2.40 (bn4a.running_var, 2.3e-7)    / 1.92 (bn4a.bias, 1.5e-6)
    b1_8x16     3.24 (descriptors, 7.5e-2 against ATen's 2.3e-2)   / 3.52 (bn4a.weight, 0.33 against 0.094)
    chain       - / 3.26 (bnPb.bias, 4.7e-6)
b1_8x16 has two values per channel in five layers: the problem itself amplifies every rounding about tenfold per coarse layer, ATen's
included, and its ratios move by a factor of 1.5 with any change of summation order.  They do not sit well below the bar: FACTOR stays 4.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

import superpoint_bn_ref as RB
from openglue_amd import features, synthetic as syn
from openglue_amd.superpoint import BN_NAMES, CONV_NAMES, SuperPointNetBn

pytestmark = pytest.mark.gpu

FACTOR = 4.0
BUFFERS = [f"{n}.{k}" for n in BN_NAMES for k in ("running_mean", "running_var")]


def _dev():
    return torch.device("cuda:0")


def _net(sd=None, **kw):
    net = SuperPointNetBn(**kw)
    net.load_state_dict(syn.make_superpoint_state_dict(True, seed=1) if sd is None else sd)
    return net.to(_dev())


def _describe(desc_nhwc, xy, dtype):
    Hc, Wc, D = desc_nhwc.shape
    p = (xy.to(dtype) - 4 + 0.5) / torch.tensor([Wc * 8 - 4.5, Hc * 8 - 4.5], dtype=dtype) * 2 - 1
    d = F.grid_sample(desc_nhwc.permute(2, 0, 1)[None], p.view(1, 1, -1, 2), mode="bilinear", align_corners=False)
    return F.normalize(d.view(D, -1).t(), p=2, dim=1)


def _oracle(img, xy, Gs, Gd, dtype, steps=1):
    """torch on the CPU in `dtype`: scores and descriptors at the pixels xy, the gradients of sum(scores * Gs) + sum(descriptors * Gd)
    after the first step, and the buffers after each of `steps` consecutive forward calls"""
    sd = {k: (v.detach().clone().to(dtype) if v.is_floating_point() else v.clone()) for k, v in syn.make_superpoint_state_dict(True, seed=1).items()}
    params = [f"{n}.{k}" for n in CONV_NAMES + BN_NAMES for k in ("weight", "bias")]
    for k in params:
        sd[k].requires_grad_(True)
    out = dict(buffers=[])
    for step in range(steps):
        heat, desc, new = RB.dense_train(sd, img, dtype=dtype)
        if step == 0:
            sc = torch.stack([heat[b, xy[b, :, 1].long(), xy[b, :, 0].long()] for b in range(img.shape[0])])
            de = torch.stack([_describe(desc[b], xy[b], dtype) for b in range(img.shape[0])])
            out["scores"], out["desc"] = sc.detach(), de.detach()
            if Gs is not None:
                ((sc * Gs.to(dtype)).sum() + (de * Gd.to(dtype)).sum()).backward()
                out["grads"] = {k: sd[k].grad for k in params}
        sd.update(new)
        out["buffers"].append({k: new[k].detach() for k in BUFFERS})
    return out


def _gpu_grads(net):
    return {f"{n}.{k}": getattr(getattr(net, n), k).grad for n in CONV_NAMES + BN_NAMES for k in ("weight", "bias")}


def _buffers(net):
    return {k: v.detach().clone() for k, v in net.state_dict().items() if "running" in k or "tracked" in k}


def _cotangents(B, n, seed=3):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, n, generator=g, dtype=torch.float64), torch.randn(B, n, 256, generator=g, dtype=torch.float64)


def _step(net, img, Gs=None, Gd=None):
    lafs, scores, desc = net(img.to(_dev()))
    if Gs is None:
        Gs, Gd = _cotangents(img.shape[0], scores.shape[1])
    (scores * Gs.to(_dev(), torch.float32)).sum().add((desc * Gd.to(_dev(), torch.float32)).sum()).backward()
    torch.cuda.synchronize()
    return lafs.detach(), scores, desc, Gs, Gd


@functools.lru_cache(maxsize=None)
def _run(case):
    """Two train-mode steps of a case (the first with a backward), shared and left unchanged by the tests that need them."""
    c = RB.CASES[case]
    img = RB.images(case)
    net = _net(**c["kw"]).train()
    lafs, scores, desc, Gs, Gd = _step(net, img)
    grad_fns = (lafs.grad_fn, scores.grad_fn, desc.grad_fn)
    buf1 = _buffers(net)
    with torch.no_grad():
        quiet = net(img.to(_dev()))
    buf2 = _buffers(net)
    return dict(net=net, img=img, lafs=lafs, scores=scores.detach(), desc=desc.detach(), Gs=Gs, Gd=Gd, grads=_gpu_grads(net), buf1=buf1,
                buf2=buf2, grad_fns=grad_fns, quiet=quiet)


@functools.lru_cache(maxsize=None)
def _oracles(case):
    r = _run(case)
    xy = r["lafs"][..., 2].cpu()
    return _oracle(r["img"], xy, r["Gs"], r["Gd"], torch.float64, 2), _oracle(r["img"], xy, r["Gs"], r["Gd"], torch.float32, 2)


def _compare(name, gpu, t64, t32):
    """prints every tensor's figures, then asserts the bar"""
    bad = []
    for k in t64:
        den = t64[k].abs().max().item()
        e_gpu = (gpu[k].detach().cpu().double() - t64[k]).abs().max().item() / den
        e_aten = (t32[k].double() - t64[k]).abs().max().item() / den
        print(f"{name} {k:22s} max {den:.3e}  gpu {e_gpu:.2e}  aten-fp32 {e_aten:.2e}  ratio {e_gpu / max(e_aten, 1e-30):.2f}")
        if not e_gpu <= FACTOR * e_aten:
            bad.append((k, e_gpu, e_aten))
    assert not bad, f"{name}: error above {FACTOR} x ATen-fp32: {bad}"


@pytest.mark.parametrize("case", list(RB.CASES))
def test_works_at_all(case):
    """NotImplementedError before this path existed"""
    r = _run(case)
    B, n = r["scores"].shape
    assert n >= (2 if case == "b1_8x16" else 8), f"{n} keypoints"
    assert r["desc"].shape == (B, n, 256) and r["lafs"].shape == (B, n, 2, 3)
    assert r["grad_fns"][0] is None and r["grad_fns"][1] is not None and r["grad_fns"][2] is not None
    assert len(r["grads"]) == 48
    for k, g in r["grads"].items():
        assert g is not None and g.shape == r["net"].state_dict()[k].shape and bool(torch.isfinite(g).all()), k
    for n_ in BN_NAMES:
        assert int(r["buf1"][f"{n_}.num_batches_tracked"]) == 1 and int(r["buf2"][f"{n_}.num_batches_tracked"]) == 2


@pytest.mark.parametrize("case", list(RB.CASES))
def test_forward_parity(case):
    r = _run(case)
    o64, o32 = _oracles(case)
    _compare(case, dict(scores=r["scores"], descriptors=r["desc"]), dict(scores=o64["scores"], descriptors=o64["desc"]),
             dict(scores=o32["scores"], descriptors=o32["desc"]))
    _compare(case + " step1", r["buf1"], o64["buffers"][0], o32["buffers"][0])
    _compare(case + " step2", r["buf2"], o64["buffers"][1], o32["buffers"][1])


@pytest.mark.parametrize("case", list(RB.CASES))
def test_gradient_parity(case):
    r = _run(case)
    o64, o32 = _oracles(case)
    keep = [k for k in o64["grads"] if not (k.startswith("conv") and k.endswith(".bias"))]
    _compare(case, r["grads"], {k: o64["grads"][k] for k in keep}, {k: o32["grads"][k] for k in keep})
    for n in CONV_NAMES:
        assert not r["grads"][f"{n}.bias"].any(), n                                   # exact zeros, not computed


def test_determinism():
    first = _run("b2_44x60")
    net = _net().train()
    lafs, scores, desc, _, _ = _step(net, first["img"], first["Gs"], first["Gd"])
    assert torch.equal(lafs, first["lafs"]) and torch.equal(scores.detach(), first["scores"]) and torch.equal(desc.detach(), first["desc"])
    for k, g in _gpu_grads(net).items():
        assert torch.equal(g, first["grads"][k]), k
    for k, v in _buffers(net).items():
        assert torch.equal(v, first["buf1"][k]), k


def test_no_grad_in_train_mode():
    """batch statistics, moved buffers, no grad_fn: the second call of _run was made under no_grad from the state after step 1, and a
    call with grad enabled from that state gives the same bits"""
    r = _run("b2_44x60")
    assert all(t.grad_fn is None and not t.requires_grad for t in r["quiet"])
    net = _net().train()
    _step(net, r["img"], r["Gs"], r["Gd"])
    out = net(r["img"].to(_dev()))
    assert out[1].grad_fn is not None
    for a, b in zip(r["quiet"], out):
        assert torch.equal(a, b.detach())
    for k, v in _buffers(net).items():
        assert torch.equal(v, r["buf2"][k]), k
    assert not torch.equal(r["buf2"]["bn1a.running_mean"], r["buf1"]["bn1a.running_mean"])
    ev = _net().eval()(r["img"].to(_dev()))                                           # running statistics instead: other values
    assert ev[1].shape != r["scores"].shape or not torch.equal(ev[1], r["scores"])


def test_eval_after_train_step_and_eval_untouched():
    """the kernels move the running buffers through raw pointers: the eval-mode blob, cached on tensor versions, must not be served stale"""
    img = RB.images("b2_44x60").to(_dev())
    net = _net()
    before = net.eval()(img)
    fresh0 = _net().eval()(img)
    assert all(torch.equal(a, b) for a, b in zip(before, fresh0))
    net.train()
    with torch.no_grad():
        net(img)
    after = net.eval()(img)
    fresh = _net(sd=net.state_dict()).eval()(img)
    assert all(a.shape == b.shape and torch.equal(a, b) for a, b in zip(after, fresh))
    assert after[1].shape != before[1].shape or not torch.equal(after[1], before[1])


def test_refusals():
    with pytest.raises(ValueError, match="more than one value per channel"):
        _net().train()(torch.zeros(1, 1, 8, 8, device=_dev()))
    net = _net().train()
    net.bn3a.momentum = None
    with pytest.raises(ValueError, match="momentum"):
        net(torch.zeros(1, 1, 16, 16, device=_dev()))
    net = _net().train()
    net.bnPb.track_running_stats = False
    with pytest.raises(ValueError, match="track_running_stats"):
        net(torch.zeros(1, 1, 16, 16, device=_dev()))


@pytest.mark.parametrize("which", ["bn", "convDb"])
def test_requires_grad_subsets(which):
    r = _run("b2_44x60")
    net = _net().train()
    wanted = (lambda name: name.startswith("bn")) if which == "bn" else (lambda name: name.startswith("convDb"))
    for name, p in net.named_parameters():
        p.requires_grad_(wanted(name))
    _step(net, r["img"], r["Gs"], r["Gd"])
    for name, p in net.named_parameters():
        if wanted(name):
            assert torch.equal(p.grad, r["grads"][name]), name
        else:
            assert p.grad is None, name


def test_no_keypoints():
    net = _net(keypoint_threshold=2.0).train()
    before = _buffers(net)
    lafs, scores, desc = net(RB.images("b2_44x60").to(_dev()))
    assert lafs.shape == (2, 0, 2, 3) and scores.shape == (2, 0) and desc.shape == (2, 0, 256)
    (scores.sum() + desc.sum()).backward()
    for p in net.parameters():
        assert p.grad is not None and p.grad.shape == p.shape and not p.grad.any()
    after = _buffers(net)
    assert all(not torch.equal(after[k], before[k]) for k in after)


def test_layer_grads_are_dense_behind_a_pool():
    """dz of a pooled layer: the pool routes gy to one pixel in four, the mean and projection terms reach every pixel -- also the row and
    column the third pool dropped"""
    c = RB.CASES["b2_44x60"]
    net = _net().train()
    net.keep_layer_grads = True
    _step(net, RB.images("b2_44x60"))
    g = net.layer_grads["conv3b"]
    assert g.shape == (2, 11, 15, 128)
    assert float((g != 0).float().mean()) > 0.99 and float(g[:, 10].abs().max()) > 0 and float(g[:, :, 14].abs().max()) > 0
    assert net.layer_grads["conv1a"].shape == (2, 44, 60, 64) and net.layer_grads["heads"].shape == (2, 5, 7, 512)
    # sum over the batch of dz and of dz * xhat vanish: what the BatchNorm backward projects out (here: the plain sum, against its scale)
    s = g.double().sum(dim=(0, 1, 2)).abs().max().item()
    assert s <= 1e-4 * g.double().abs().sum(dim=(0, 1, 2)).max().item()


def test_chain_through_superglue():
    """extractor -> prepare_features_output -> SuperGlue.train() -> loss: the gradients the matcher hands back, fed to the float64
    oracle as Gs / Gd, reproduce the extractor's parameter gradients under the same rule"""
    from openglue_amd.superglue import SuperGlue
    H, W = 72, 136
    base = RB.images("b1_72x136")
    img = torch.cat([base, torch.roll(base, -8, dims=3)])
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
    o64, o32 = _oracle(img, xy, Gs, Gd, torch.float64), _oracle(img, xy, Gs, Gd, torch.float32)
    keep = [k for k in o64["grads"] if not (k.startswith("conv") and k.endswith(".bias"))]
    _compare("chain", _gpu_grads(net), {k: o64["grads"][k] for k in keep}, {k: o32["grads"][k] for k in keep})
