"""SuperPointNetBn fine-tuning, the parts that need no GPU: the float64 oracle of tests/superpoint_bn_ref.py against an assembly of
nn.Conv2d / nn.BatchNorm2d modules in train(), the conditions the GPU cases rest on (keypoints, pool margins, vanishing convolution-bias
gradients), and the new entry points' ABI and argument checks."""
import ctypes as C
import functools
import os
import re

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import superpoint_bn_ref as RB
import superpoint_ref as R
from openglue_amd import _lib, build, kernel_trace, synthetic as syn
from openglue_amd.superpoint import BN_NAMES, CONV_NAMES, SuperPointNetBn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = {"og_superpoint_bn_train_saved_bytes", "og_superpoint_bn_train_workspace_bytes", "og_superpoint_bn_train_forward",
               "og_superpoint_bn_cell_tail", "og_superpoint_bn_train_backward"}
E_INVALID, E_SHAPE, E_ALIGN = -1, -2, -3


class _Assembly(nn.Module):
    """the reference's SuperPointNetBn._forward_layers, from torch modules"""

    def __init__(self):
        super().__init__()
        ch = [(1, 64), (64, 64), (64, 64), (64, 64), (64, 128), (128, 128), (128, 128), (128, 128)]
        for tag, (ci, co) in zip(RB.TRUNK, ch):
            setattr(self, "conv" + tag, nn.Conv2d(ci, co, 3, padding=1))
            setattr(self, "bn" + tag, nn.BatchNorm2d(co))
        for tag, ci, co, k in (("Pa", 128, 256, 3), ("Pb", 256, 65, 1), ("Da", 128, 256, 3), ("Db", 256, 256, 1)):
            setattr(self, "conv" + tag, nn.Conv2d(ci, co, k, padding=k // 2))
            setattr(self, "bn" + tag, nn.BatchNorm2d(co))

    def forward(self, x):
        for i in range(4):
            x = F.relu(getattr(self, f"bn{i + 1}a")(getattr(self, f"conv{i + 1}a")(x)))
            x = F.relu(getattr(self, f"bn{i + 1}b")(getattr(self, f"conv{i + 1}b")(x)))
            if i != 3:
                x = F.max_pool2d(x, 2, 2)
        d = self.bnDb(self.convDb(F.relu(self.bnDa(self.convDa(x)))))
        d = d.div(torch.unsqueeze(torch.norm(d, p=2, dim=1), 1))
        s = F.softmax(self.bnPb(self.convPb(F.relu(self.bnPa(self.convPa(x))))), 1)[:, :-1]
        return d, s


def _sd64(requires_grad=True):
    sd = {k: v.detach().clone() for k, v in syn.make_superpoint_state_dict(True, seed=1).items()}
    for k, v in sd.items():
        if v.is_floating_point():
            sd[k] = v.double().requires_grad_(requires_grad and "running" not in k)
    return sd


def test_oracle_equals_torch_modules_over_two_steps():
    img = RB.images("b2_44x60").double()
    g = torch.Generator().manual_seed(0)
    sd = _sd64()
    net = _Assembly().double()
    net.load_state_dict({k: v.detach() for k, v in sd.items()})
    net.train()
    for step in range(2):
        heat, desc, new = RB.dense_train(sd, img)
        d, s = net(img)
        b, _, h, w = s.shape
        want_heat = s.permute(0, 2, 3, 1).reshape(b, h, w, 8, 8).permute(0, 1, 3, 2, 4).reshape(b, h * 8, w * 8)
        assert float((heat - want_heat).detach().abs().max()) <= 1e-12 and float((desc - d.permute(0, 2, 3, 1)).detach().abs().max()) <= 1e-12
        Gh, Gd = torch.randn(heat.shape, generator=g, dtype=torch.float64), torch.randn(desc.shape, generator=g, dtype=torch.float64)
        params = [k for k, v in sd.items() if v.requires_grad]
        got = torch.autograd.grad((heat * Gh).sum() + (desc * Gd).sum(), [sd[k] for k in params])
        net.zero_grad()
        ((want_heat * Gh).sum() + (d.permute(0, 2, 3, 1) * Gd).sum()).backward()
        want = dict(net.named_parameters())
        for k, gk in zip(params, got):
            den = max(float(want[k].grad.abs().max()), 1e-300)
            assert float((gk - want[k].grad).abs().max()) <= 1e-12 * max(den, 1.0), k
        state = net.state_dict()
        for k, v in new.items():
            if k.endswith("num_batches_tracked"):
                assert int(v) == int(state[k]) == step + 1, k
            else:
                assert float((v - state[k]).abs().max()) <= 1e-12, k
        for k, v in new.items():                     # the second step starts from the moved buffers
            sd[k] = v


@functools.lru_cache(maxsize=None)
def _oracle(case):
    c = RB.CASES[case]
    taps = {}
    sd = _sd64()
    heat, desc, _ = RB.dense_train(sd, RB.images(case), taps=taps)
    return c, sd, heat, desc, taps


@pytest.mark.parametrize("case", list(RB.CASES))
def test_case_conditions(case):
    """enough keypoints, and no pool window that fp32 and float64 could decide differently (a condition on the inputs: another seed if
    it fails, never a tolerance)"""
    c, sd, heat, desc, taps = _oracle(case)
    net = SuperPointNetBn(**c["kw"])
    sel = R.select(heat.detach(), net.nms_kernel, net.remove_borders_size, net.keypoint_threshold, net.max_keypoints)
    n = min(len(s["idx"]) for s in sel)
    print(case, "keypoints", n, "pool margin", RB.pool_margins(taps))
    assert n >= (2 if case == "b1_8x16" else 8)
    assert RB.pool_margins(taps) >= 1e-5


def test_conv_bias_gradients_vanish():
    """the mean subtraction removes every convolution bias: in float64 its gradient is rounding noise next to the layer's d beta"""
    c, sd, heat, desc, taps = _oracle("b2_44x60")
    g = torch.Generator().manual_seed(3)
    Gh, Gd = torch.randn(heat.shape, generator=g, dtype=torch.float64), torch.randn(desc.shape, generator=g, dtype=torch.float64)
    keys = [f"{n}.bias" for n in CONV_NAMES] + [f"{n}.bias" for n in BN_NAMES]
    grads = dict(zip(keys, torch.autograd.grad((heat * Gh).sum() + (desc * Gd).sum(), [sd[k] for k in keys])))
    for cn in CONV_NAMES:
        bn = "bn" + cn[4:]
        dbeta = float(grads[f"{bn}.bias"].abs().max())
        assert dbeta > 0 and float(grads[f"{cn}.bias"].abs().max()) < 1e-9 * dbeta, (cn, bn)


def test_abi_and_sizes():
    header = open(os.path.join(ROOT, "include", "openglue_amd.h")).read()
    declared = set(re.findall(r"^\s*(?:int|size_t)\s+(og_\w+)\s*\(", header, flags=re.M))
    assert NEW_SYMBOLS <= declared and declared == set(_lib.SYMBOLS)
    lib = _lib.load()
    assert all(hasattr(lib, n) for n in NEW_SYMBOLS) and lib.og_abi_version() == 14
    assert "superpoint_bn_train.hip" in build.SOURCES and "sp_bn_reduce_kernel<" in kernel_trace.SUPERPOINT_BN_TRAIN
    # the bodies shared with SuperPointNet (csrc/og_superpoint_train.h) are traced per network: neither list takes the other's instances
    shared = ("sp_dgrad_kernel<{},", "sp_wgrad_kernel<{},", "sp_wgrad1a_kernel<{}>", "sp_grad_dump_kernel<{},")
    assert all(s.format("SpBn") in kernel_trace.SUPERPOINT_BN_TRAIN and s.format("SpPlain") in kernel_trace.SUPERPOINT_TRAIN for s in shared)
    assert not any(s.format("SpPlain").startswith(kernel_trace.SUPERPOINT_BN_TRAIN) or s.format("SpBn").startswith(kernel_trace.SUPERPOINT_TRAIN)
                   for s in shared)
    assert lib.og_superpoint_bn_train_saved_bytes(1, 8, 8) == 0 and lib.og_superpoint_bn_train_workspace_bytes(1, 8, 8) == 0      # N = 1
    assert lib.og_superpoint_bn_train_saved_bytes(1, 8, 16) > 0 and lib.og_superpoint_bn_train_saved_bytes(2, 8, 8) > 0          # N = 2
    assert lib.og_superpoint_bn_train_saved_bytes(1, 7, 60) == 0 and lib.og_superpoint_bn_train_saved_bytes(1, 8192, 8193) == 0
    B, H, W = 2, 44, 60
    r = lambda n: (n + 63) // 64 * 64
    # hidden, the coefficients (4 x 1280), then the raw output of conv1a and of the eight layers at the resolution they convolve at
    want = r(B * 35 * 512) + r(4 * 1280) + r(B * 44 * 60 * 64) * 2 + r(B * 22 * 30 * 64) * 2 + r(B * 11 * 15 * 128) * 2 + r(B * 35 * 128) * 2 + \
        r(B * 35 * 512)
    assert lib.og_superpoint_bn_train_saved_bytes(B, H, W) == 4 * want
    assert lib.og_superpoint_bn_train_workspace_bytes(B, H, W) >= 4 * (B * H * W * 64 + B * 22 * 30 * 64)


def test_entry_points_refuse_bad_arguments():
    """null pointers, bad sizes and misaligned buffers come back as error codes; nothing is launched (there is no GPU here)"""
    lib = _lib.load()
    buf = (C.c_float * 64)()
    p = C.addressof(buf)
    p += (-p) % 16
    bn = (C.c_void_p * 40)(*([p] * 40))
    f10 = (C.c_float * 10)(*([0.1] * 10))
    assert lib.og_superpoint_bn_train_forward(1, 16, 16, None, p, bn, f10, f10, p, p, None) == E_INVALID
    assert lib.og_superpoint_bn_train_forward(1, 8, 8, p, p, bn, f10, f10, p, p, None) == E_SHAPE
    assert lib.og_superpoint_bn_train_forward(1, 16, 16, p, p + 4, bn, f10, f10, p, p, None) == E_ALIGN
    bn[7] = None
    assert lib.og_superpoint_bn_train_forward(1, 16, 16, p, p, bn, f10, f10, p, p, None) == E_INVALID
    assert lib.og_superpoint_bn_train_backward(1, 16, 16, p, p, p, p, 0, p, None, None, p, None) == E_INVALID
    assert lib.og_superpoint_bn_train_backward(1, 16, 16, p, p, p, p, 9, p, p, None, p, None) == E_SHAPE
    assert lib.og_superpoint_bn_train_backward(1, 8, 8, p, p, p, p, 0, p, p, None, p, None) == E_SHAPE
    assert lib.og_superpoint_bn_train_backward(1, 16, 16, p, p, p, p + 4, 0, p, p, None, p, None) == E_ALIGN
    assert lib.og_superpoint_bn_cell_tail(1, 2, 2, p, 64, p, p, p, None) == E_SHAPE
    assert lib.og_superpoint_bn_cell_tail(1, 2, 2, None, 68, p, p, p, None) == E_INVALID


def test_python_refusals():
    img = torch.zeros(1, 1, 16, 16)
    with pytest.raises(NotImplementedError, match="no CPU path for training-mode BatchNorm"):
        SuperPointNetBn().train()(img)
    with pytest.raises(RuntimeError, match="no CPU path"):                            # eval(): device handling unchanged
        SuperPointNetBn().eval()(img)
