"""The fragment-major weight layout of the fp32 MFMA convolutions (csrc/og_conv_f32.h: pack_fragments), restated once in numpy and
read back from all five packed blobs: SuperPoint with and without BatchNorm, HardNet, AffNet, OriNet.  Every folded 3x3, cell and
tail weight must come back as float32(float64(w) * scale), bit for bit, and the padded rows must be zero.  No GPU."""
import ctypes as C

import numpy as np
import pytest
import torch

from openglue_amd import _lib, synthetic as syn
from openglue_amd import affnet_hardnet as ah
from openglue_amd.superpoint import methods


def unpack_fragments(blob, rows_padded, K):
    """W[co][k] of a [rows_padded][K] matrix stored as [jt][step][lane][4]: lane l of tile jt, step s holds
    W[32 jt + (l & 31)][8 s + 4 (l >> 5) + e]"""
    assert blob.size == rows_padded * K and rows_padded % 32 == 0 and K % 8 == 0
    co, k = np.arange(rows_padded)[:, None], np.arange(K)[None, :]
    s, h, e = k // 8, (k % 8) // 4, k % 4
    return blob[(((co // 32) * (K // 8) + s) * 64 + (co & 31) + 32 * h) * 4 + e]


def conv3x3_k(cin, kc):
    """(ci, tap) of every k of a 3x3 layer staged kc channels at a time: step = (chunk * 9 + tap) * (kc / 8) + kk"""
    k = np.arange(9 * cin)
    s, spc = k // 8, 9 * (kc // 8)
    return (s // spc) * kc + (s % (kc // 8)) * 8 + k % 8, (s % spc) // (kc // 8)


def folded(w, scale):
    """float32(float64(w) * scale) per output row"""
    return (w.astype(np.float64) * np.asarray(scale, np.float64).reshape(-1, *([1] * (w.ndim - 1)))).astype(np.float32)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def check_conv3x3(blob, w, scale, kc, cout_padded):
    cout, cin = w.shape[:2]
    got = unpack_fragments(blob, cout_padded, 9 * cin)
    ci, tap = conv3x3_k(cin, kc)
    assert sorted(zip(ci.tolist(), tap.tolist())) == [(c, t) for c in range(cin) for t in range(9)]      # every weight once
    assert same_bits(got[:cout], folded(w, scale).reshape(cout, cin, 9)[:, ci, tap])
    assert same_bits(got[cout:], np.zeros((cout_padded - cout, 9 * cin), np.float32))


def _pack(fn, args, tensors, nbytes):
    host = [t.detach().to("cpu", torch.float32).contiguous() for t in tensors]
    ptrs = (C.c_void_p * len(host))(*[h.data_ptr() for h in host])
    blob = torch.full((nbytes // 4,), float("nan"), dtype=torch.float32)       # the packer writes every float
    assert fn(*args, ptrs, blob.data_ptr()) == 0
    return blob.numpy(), [h.numpy() for h in host]


@pytest.mark.parametrize("bn", [False, True])
def test_superpoint_blob(bn):
    lib = _lib.load()
    net = methods["SuperPointNetBn" if bn else "SuperPointNet"]()
    net.load_state_dict(syn.make_superpoint_state_dict(bn, seed=7), strict=True)
    eps = float(net.bn1a.eps) if bn else 0.0
    blob, host = _pack(lib.og_superpoint_pack, (256, int(bn), eps), net._pack_tensors(), lib.og_superpoint_packed_bytes(256))
    assert np.isfinite(blob).all()

    def scale(conv):                      # conv 0..11 in the order conv1a .. conv4b, convPa, convPb, convDa, convDb
        if not bn:
            return np.ones(host[2 * conv].shape[0])
        gamma, var = host[24 + 4 * conv], host[24 + 4 * conv + 3]
        return gamma.astype(np.float64) / np.sqrt(var.astype(np.float64) + np.float64(np.float32(eps)))

    cin = [64, 64, 64, 64, 128, 128, 128, 128]
    cout = [64, 64, 64, 128, 128, 128, 128, 512]
    o = 9 * 64 + 64                                                           # conv1a runs on the VALU: [tap][64], then its bias
    for l in range(8):
        n = cout[l] * 9 * cin[l]
        if l < 7:
            w, sc = host[2 * (l + 1)], scale(l + 1)
        else:                                                                 # convPa | convDa in one launch
            w, sc = np.concatenate([host[16], host[20]]), np.concatenate([scale(8), scale(10)])
        check_conv3x3(blob[o:o + n], w, sc, 32, cout[l])
        o += n + cout[l]
    logits = unpack_fragments(blob[o:o + 96 * 256], 96, 256)                  # convPb: 65 rows in three tiles
    assert same_bits(logits[:65], folded(host[18].reshape(65, 256), scale(9)))
    assert same_bits(logits[65:], np.zeros((31, 256), np.float32))
    o += 96 * 256
    assert same_bits(unpack_fragments(blob[o:o + 256 * 256], 256, 256), folded(host[22].reshape(256, 256), scale(11)))
    o += 256 * 256
    assert same_bits(blob[o + 65:o + 96], np.zeros(31, np.float32)) and o + 96 + 256 == blob.size


@pytest.mark.parametrize("kind", ["hardnet", "affnet", "orinet"])
def test_patchnet_blob(kind):
    lib = _lib.load()
    net = {"hardnet": ah.HardNet, "affnet": ah.AffNet, "orinet": ah.OriNet}[kind]()
    net.load_state_dict(syn.make_patchnet_state_dict(kind, seed=7), strict=True)
    eps = float(net.features[1].eps)
    blob, host = _pack(lib.og_patchnet_pack, (ah.KINDS[kind], eps), net._pack_tensors(), lib.og_patchnet_packed_bytes(ah.KINDS[kind]))
    assert np.isfinite(blob).all()

    def scale(var):
        return 1.0 / np.sqrt(var.astype(np.float64) + np.float64(np.float32(eps)))

    c = 32 if kind == "hardnet" else 16
    o = 10 * c                                                                # conv0 runs on the VALU: [tap][c], then its bias
    for l, (ci, co, stride) in enumerate([(c, c, 1), (c, 2 * c, 2), (2 * c, 2 * c, 1), (2 * c, 4 * c, 2), (4 * c, 4 * c, 1)]):
        cop = max(co, 32)
        kc = 16 if stride == 2 or ci == 16 else 32
        w, var = host[3 * (l + 1)], host[3 * (l + 1) + 2]
        assert w.shape == (co, ci, 3, 3)
        check_conv3x3(blob[o:o + cop * 9 * ci], w, scale(var), kc, cop)
        o += cop * 9 * ci
        assert same_bits(blob[o + co:o + cop], np.zeros(cop - co, np.float32))                     # padded bias
        o += cop
    C4, nout = 4 * c, host[18].shape[0]
    K = 64 * C4
    w_k = host[18].reshape(nout, C4, 64).transpose(0, 2, 1).reshape(nout, K)                      # k = (y * 8 + x) * C + c
    if kind == "hardnet":
        assert same_bits(unpack_fragments(blob[o:o + 128 * K], 128, K), folded(w_k, scale(host[20])))
    else:
        assert same_bits(blob[o:o + nout * K].reshape(nout, K), w_k)                               # VALU tail: plain rows, no fold
    assert o + nout * K + (nout + 3) // 4 * 4 == blob.size


def test_layout_formula_on_one_fragment():
    """one tile, one step: lane l = co + 32 h holds the four floats k = 4 h .. 4 h + 3 of row co"""
    back = unpack_fragments(np.arange(32 * 8, dtype=np.float32), 32, 8)
    assert back[3].tolist() == [12, 13, 14, 15, 140, 141, 142, 143]
