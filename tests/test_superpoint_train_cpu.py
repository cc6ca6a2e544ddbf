"""SuperPoint fine-tuning, the parts that need no GPU: the ABI (header == binding, version, source list), the argument checks of the new
entry points (refused before anything is launched), and the data-gradient weight blob of og_superpoint_train_pack -- weights transposed
(Cin and Cout swapped) and taps flipped in the fragment-major layout of og_conv_f32.h -- read back against a numpy restatement."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from openglue_amd import _lib, build, synthetic as syn
from openglue_amd.superpoint import CONV_NAMES, SuperPointNet, SuperPointNetBn, _GRAD_FLOATS, _GRAD_SLICES
from test_attention_resources_cpu import _compile
from test_fragment_packing_cpu import _pack, conv3x3_k, same_bits, unpack_fragments

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = {"og_superpoint_train_packed_bytes", "og_superpoint_train_pack", "og_superpoint_train_saved_bytes",
               "og_superpoint_train_workspace_bytes", "og_superpoint_train_forward", "og_superpoint_train_backward",
               "og_superpoint_describe_backward"}
E_INVALID, E_SHAPE, E_ALIGN = -1, -2, -3
# the eight MFMA layers: (Cin, Cout); the last is convPa | convDa as one layer
LAYERS = [(64, 64), (64, 64), (64, 64), (64, 128), (128, 128), (128, 128), (128, 128), (128, 512)]


def test_abi():
    header = open(os.path.join(ROOT, "include", "openglue_amd.h")).read()
    declared = set(re.findall(r"^\s*(?:int|size_t)\s+(og_\w+)\s*\(", header, flags=re.M))
    assert NEW_SYMBOLS <= declared and NEW_SYMBOLS <= set(_lib.SYMBOLS)
    assert declared == set(_lib.SYMBOLS), declared ^ set(_lib.SYMBOLS)
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
    assert _lib.OG_ABI_VERSION == 14 and lib.og_abi_version() == 14
    assert re.search(r"#define\s+OG_ABI_VERSION\s+14\b", header)
    assert "superpoint_train.hip" in build.SOURCES


def test_sizes():
    lib = _lib.load()
    assert lib.og_superpoint_train_packed_bytes(256) == 4 * sum(ci * co * 9 for ci, co in LAYERS)
    assert lib.og_superpoint_train_packed_bytes(128) == 0
    assert lib.og_superpoint_train_saved_bytes(0, 44, 60) == 0 and lib.og_superpoint_train_saved_bytes(1, 7, 60) == 0
    assert lib.og_superpoint_train_saved_bytes(1, 8192, 8193) == 0                    # B * H * W > 2^26
    assert lib.og_superpoint_train_workspace_bytes(1, 44, 60, -1) == 0 and lib.og_superpoint_train_workspace_bytes(1, 4, 60, 8) == 0
    # hidden [Hc Wc][512] + conv1a + (pre, pooled) x 3 + four unpooled layers, each rounded up to 64 floats
    B, H, W = 2, 44, 60
    r = lambda n: (n + 63) // 64 * 64
    want = r(B * 5 * 7 * 512) + r(B * 44 * 60 * 64) * 2 + r(B * 22 * 30 * 64) * 3 + r(B * 11 * 15 * 64) + r(B * 11 * 15 * 128) * 2 + \
        r(B * 5 * 7 * 128) * 3
    assert lib.og_superpoint_train_saved_bytes(B, H, W) == 4 * want
    ws = lib.og_superpoint_train_workspace_bytes(B, H, W, 21)
    assert ws >= 4 * (B * H * W * 64 + B * 22 * 30 * 64) and ws >= 4 * B * 21 * 262
    # the flat gradient buffer of the Python side mirrors the C layout: every parameter once, nothing overlapping
    spans = sorted((o, o + int(np.prod(s))) for name in CONV_NAMES if name in _GRAD_SLICES for o, s in _GRAD_SLICES[name])
    assert spans[0][0] == 0 and spans[-1][1] == _GRAD_FLOATS and all(a[1] == b[0] for a, b in zip(spans, spans[1:]))


def test_entry_points_refuse_bad_arguments():
    """null pointers, bad sizes and misaligned buffers come back as error codes; nothing is launched (there is no GPU here)"""
    lib = _lib.load()
    buf = torch.zeros(4096, dtype=torch.float32)
    p = buf.data_ptr()
    assert p % 16 == 0
    fwd = lambda **k: lib.og_superpoint_train_forward(*[{**dict(b=1, H=44, W=60, img=p, pk=p, sv=p, heat=p, desc=p, st=None), **k}[n]
                                                        for n in ("b", "H", "W", "img", "pk", "sv", "heat", "desc", "st")])
    for name in ("img", "pk", "sv", "heat", "desc"):
        assert fwd(**{name: None}) == E_INVALID, name
    assert fwd(b=0) == E_SHAPE and fwd(H=7) == E_SHAPE and fwd(W=4) == E_SHAPE and fwd(H=8192, W=8193) == E_SHAPE
    assert fwd(pk=p + 4) == E_ALIGN and fwd(sv=p + 4) == E_ALIGN and fwd(desc=p + 8) == E_ALIGN

    bwd = lambda **k: lib.og_superpoint_train_backward(*[{**dict(b=1, H=44, W=60, img=p, pg=p, sv=p, gh=p, first=0, gr=p, dbg=None, ws=p,
                                                                 st=None), **k}[n]
                                                         for n in ("b", "H", "W", "img", "pg", "sv", "gh", "first", "gr", "dbg", "ws", "st")])
    for name in ("img", "pg", "sv", "gh", "gr", "ws"):
        assert bwd(**{name: None}) == E_INVALID, name
    assert bwd(b=-1) == E_SHAPE and bwd(H=3) == E_SHAPE and bwd(first=-1) == E_SHAPE and bwd(first=9) == E_SHAPE
    assert bwd(pg=p + 4) == E_ALIGN and bwd(gh=p + 4) == E_ALIGN and bwd(ws=p + 8) == E_ALIGN and bwd(dbg=p + 4) == E_ALIGN

    dsc = lambda **k: lib.og_superpoint_describe_backward(*[{**dict(b=1, Hc=5, Wc=7, n=8, idx=p, ld=8, cd=p, dd=p, dc=p, ws=p, st=None), **k}[n]
                                                            for n in ("b", "Hc", "Wc", "n", "idx", "ld", "cd", "dd", "dc", "ws", "st")])
    for name in ("idx", "cd", "dd", "dc", "ws"):
        assert dsc(**{name: None}) == E_INVALID, name
    assert dsc(b=0) == E_SHAPE and dsc(Hc=0) == E_SHAPE and dsc(n=0) == E_SHAPE and dsc(ld=7) == E_SHAPE
    assert dsc(cd=p + 4) == E_ALIGN and dsc(dd=p + 4) == E_ALIGN and dsc(dc=p + 4) == E_ALIGN

    ptrs = (C.c_void_p * 24)(*([p] * 24))
    assert lib.og_superpoint_train_pack(128, ptrs, p) == E_SHAPE
    assert lib.og_superpoint_train_pack(256, None, p) == E_INVALID and lib.og_superpoint_train_pack(256, ptrs, None) == E_INVALID
    ptrs[5] = None
    assert lib.og_superpoint_train_pack(256, ptrs, p) == E_INVALID


def test_dgrad_blob_round_trip():
    """unpack every layer's block, un-transpose and un-flip it: the module's weights, bit for bit"""
    lib = _lib.load()
    net = SuperPointNet()
    net.load_state_dict(syn.make_superpoint_state_dict(False, seed=1))
    blob, host = _pack(lib.og_superpoint_train_pack, (256,), net._pack_tensors(), lib.og_superpoint_train_packed_bytes(256))
    assert not np.isnan(blob).any()
    weights = {name: host[2 * i] for i, name in enumerate(CONV_NAMES)}
    o = 0
    for j, (cin, cout) in enumerate(LAYERS):
        w = weights[CONV_NAMES[j + 1]] if j < 7 else np.concatenate([weights["convPa"], weights["convDa"]])      # [cout][cin][3][3]
        assert w.shape == (cout, cin, 3, 3)
        got = unpack_fragments(blob[o:o + cin * cout * 9], cin, 9 * cout)            # rows = the layer's INPUT channels, K = 9 x output channels
        co, tap = conv3x3_k(cout, 32)
        assert sorted(zip(co.tolist(), tap.tolist())) == [(c, t) for c in range(cout) for t in range(9)]
        back = np.zeros((cout, cin, 9), np.float32)
        back[co, :, 8 - tap] = got.T                                                  # blob tap t' is weight tap 8 - t'
        assert same_bits(back, w.reshape(cout, cin, 9)), CONV_NAMES[j + 1] if j < 7 else "heads"
        o += cin * cout * 9
    assert o == blob.size


def test_training_kernels_do_not_spill_and_reach_their_occupancy(tmp_path):
    usage, need = _compile("superpoint_train.hip", tmp_path)
    mine = {k: u for k, u in usage.items() if any(t in k for t in ("dgrad", "wgrad", "save_kernel", "reduce_parts", "describe_bwd", "grad_dump"))}
    assert len(mine) == 14, sorted(mine)             # 2 save, 4 dgrad, 2 wgrad, wgrad1a, reduce, 2 describe, 2 dump
    bad = []
    for k, u in sorted(usage.items()):               # the unit's instances of the inference kernels included
        occ = int(u["Occupancy [waves/SIMD]"])
        print(f"{k}: VGPRs {u['VGPRs']} AGPRs {u['AGPRs']} scratch {u['ScratchSize [bytes/lane]']} spill {u['VGPRs Spill']} occupancy {occ} >= {need[k]}")
        if int(u["ScratchSize [bytes/lane]"]) != 0 or int(u["VGPRs Spill"]) != 0 or occ < need[k]:
            bad.append((k, u, need[k]))
    assert not bad, bad


def test_packed_grad_follows_the_weights():
    """_pack_grad's key: an in-place update (an optimizer step) bumps _version -> the blob is rebuilt, as _pack"""
    net = SuperPointNet()
    key = lambda: tuple((t.data_ptr(), t._version) for t in net._pack_tensors())
    k0 = key()
    with torch.no_grad():
        net.conv3a.weight.mul_(0.5)
    assert key() != k0


def test_bn_variant_still_refuses_training():
    net = SuperPointNetBn().train()
    with pytest.raises(NotImplementedError):
        net(torch.zeros(1, 1, 16, 16))
    with pytest.raises(RuntimeError, match="no CPU path"):                            # SuperPointNet in train(): device handling unchanged
        SuperPointNet().train()(torch.zeros(1, 1, 16, 16))
