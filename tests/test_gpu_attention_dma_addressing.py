"""The scalar-addressed K/V DMA of attention_dma_kernel (csrc/attention.hip) at every tile count and clamp position.

The kernel fetches a 64-key tile with plane bases held in scalar registers that advance once per tile, plus a loop-invariant lane offset;
only the fetch of a problem's LAST tile clamps its rows (rows past the last key would lie outside the problem).  Which code fetches the
last tile depends on the tile count: tile 0's prologue (one tile), tile 0's step (two), the steps behind the pair loop (three and more),
into either LDS buffer.  The cases:

  a. key counts {1, 63, 64, 65, 128, 129, 191} x query counts {1, 127, 129} at dh = 64 and dh = 32, two problems x four heads: the
     4-wave batch form at one, two and three tiles, with a clamped last tile in either buffer and a one-tile problem whose prologue tile
     is also the masked one; ops.attention against float64 softmax attention at the tolerance of test_gpu_parity.test_attention_vs_oracle;
  b. the key split (KS = 2) once: both halves end in a clamped tile;
  c. a ragged batch through the packed path (og_forward_ragged) with unequal per-pair lengths -- every pair's first K/V row is a non-zero,
     non-tile-aligned row of the packed matrix -- at sizes that choose the grid split GS = 2 and GS = 4 (and GS = 4 at dh = 32), each
     pair against the float64 oracle at the tolerance of the other ragged tests;
  d. a cross-shaped problem (nq != nk) read from q|k|v planes with row stride 3 D and head offset h dh inside the row, the layout
     og_forward projects into, through lib.og_attention.

Every case asserts the attention instances it launched (tests/test_gpu_attention_dispatch.py's restatement of the dispatch rule).
"""
import pytest
import torch

from openglue_amd import _lib, ops, synthetic as syn
from oracle import superglue_oracle as orc
from tests.test_gpu_attention_dispatch import KS64, _ref, _traced, expected_instance, forward_instances
from tests.test_gpu_parity import TOL_SCORES, _build
from tests.util import MATCH_THRESHOLD, to_device

pytestmark = pytest.mark.gpu

TOL_O = 5e-5                  # test_attention_vs_oracle: split-f16 operands, ~22 mantissa bits per product
NKS = (1, 63, 64, 65, 128, 129, 191)
NQS = (1, 127, 129)
LOG2E = 1.4426950408889634


def _inputs(Z, nq, nk, H, dh, seed):
    g = torch.Generator().manual_seed(seed)
    D = H * dh
    q, k, v = torch.randn(Z, nq, D, generator=g) * 3.0, torch.randn(Z, nk, D, generator=g) * 3.0, torch.randn(Z, nk, D, generator=g) * 2.0
    return q * dh ** -0.5, k, v


@pytest.fixture(scope="module")
def batch_form_references():
    """float64 results of the whole matrix, computed once"""
    out = {}
    for dh in (64, 32):
        for nk in NKS:
            for nq in NQS:
                qs, k, v = _inputs(2, nq, nk, 4, dh, nq * 7919 + nk * 31 + dh)
                out[dh, nk, nq] = (qs, k, v, _ref(qs, k, v, 4)[0])
    return out


@pytest.mark.parametrize("dh", [64, 32])
@pytest.mark.parametrize("nk", NKS)
def test_batch_form_tile_counts_and_clamps(gpu_device, batch_form_references, dh, nk):
    H = 4
    want = f"attention_dma_kernel<{dh}, RaggedNone, 1, 1, 0, 0>"
    for nq in NQS:
        assert expected_instance(2, H, dh, nq, nk) == want
        qs, k, v, O = batch_form_references[dh, nk, nq]
        o, inst, _ = _traced(lambda: ops.attention(qs.to(gpu_device), k.to(gpu_device), v.to(gpu_device), H))
        assert inst == {want}, (inst, want)
        o = o.cpu()
        err = (o.double() - O).abs().max().item()
        print(f"[dma addressing dh={dh} nq={nq} nk={nk}] {want}: max |O - float64| {err:.2e} (bound {TOL_O:.1e})")
        assert torch.isfinite(o).all(), (nq, nk)
        assert err < TOL_O, (nq, nk, err)


def test_key_split_halves_end_in_clamped_tiles(gpu_device):
    """321 keys = 6 tiles: half 0 walks tiles 0..2, half 1 tiles 3..5, the last of them with one key"""
    H, dh, nq, nk = 4, 64, 129, 321
    assert expected_instance(2, H, dh, nq, nk) == KS64
    qs, k, v = _inputs(2, nq, nk, H, dh, 77)
    o, inst, _ = _traced(lambda: ops.attention(qs.to(gpu_device), k.to(gpu_device), v.to(gpu_device), H))
    assert inst == {KS64}, inst
    err = (o.cpu().double() - _ref(qs, k, v, H)[0]).abs().max().item()
    print(f"[dma addressing key split nq={nq} nk={nk}] max |O - float64| {err:.2e}")
    assert err < TOL_O, err


RAGGED_LENS = [(300, 129), (65, 257), (191, 64), (130, 321)]


@pytest.mark.parametrize("D,forms", [(256, ("RaggedDesc, 1, 2, 0, 0>", "RaggedDesc, 1, 4, 0, 0>")), (128, ("RaggedDesc, 1, 4, 0, 0>",))])
def test_ragged_packed_rows_and_grid_split(gpu_device, D, forms):
    """Four pairs of unequal sizes: the self layer (8 problems x 4 heads x 3 query tiles = 96 workgroups) takes GS = 2 at dh = 64, the
    cross layers (48) GS = 4; every pair's keys start at a row of the packed matrix that is no multiple of 64."""
    H, dh = 4, D // 4
    cfg = syn.make_config(descriptor_dim=D, num_stages=2, num_heads=H, num_iters=20, side_info_size=1)
    sd = syn.make_state_dict(cfg, seed=0)
    model = _build(cfg, sd, gpu_device)
    pairs_cpu = []
    for i, (m, n) in enumerate(RAGGED_LENS):
        p = syn.make_pair(m, n, D, 1, seed=900 + i)
        p["image0_size"] = list(syn.IMAGE_WH); p["image1_size"] = list(syn.IMAGE_WH)
        pairs_cpu.append(p)
    pairs = [to_device(p, gpu_device) for p in pairs_cpu]
    res, inst, _ = _traced(lambda: model.match_ragged(pairs, MATCH_THRESHOLD))
    want = forward_instances(len(RAGGED_LENS), max(m for m, _ in RAGGED_LENS), max(n for _, n in RAGGED_LENS), H, dh, ragged=True)
    assert inst == want, (inst, want)
    for f in forms:
        assert any(w.endswith(f) for w in want), (f, want)
    for p, r, (m, n) in zip(pairs_cpu, res, RAGGED_LENS):
        s = r["scores"].cpu()
        assert s.shape == (m + 1, n + 1) and torch.isfinite(s).all(), (m, n)
        one = {k: (v[None] if torch.is_tensor(v) else v) for k, v in p.items()}
        with torch.no_grad():
            o64 = orc.superglue_forward(sd, cfg, one, dtype=torch.float64)
        err = (s.double() - o64["scores"][0]).abs().max().item()
        print(f"[dma addressing ragged D={D} pair {m}x{n}] scores err {err:.2e} (bound {TOL_SCORES:.1e})")
        assert err < TOL_SCORES, ((m, n), err)


@pytest.mark.parametrize("dh", [64, 32])
def test_cross_shape_from_qkv_planes(gpu_device, dh):
    """Queries of one image against keys of the other, each read from its image's [n, q | k | v] planes: ld = 3 D, k at column D, v at 2 D"""
    lib = _lib.load()
    Z, H, nq, nk = 2, 4, 129, 191
    D = H * dh
    qs, k, v = _inputs(Z, nq, nk, H, dh, 5 + dh)
    dev = gpu_device
    want = expected_instance(Z, H, dh, nq, nk)
    assert want == f"attention_dma_kernel<{dh}, RaggedNone, 1, 1, 0, 0>"
    g = torch.Generator().manual_seed(1)
    planes0 = [torch.randn(Z, nq, 3 * D, generator=g).to(dev).half() for _ in range(2)]      # image 0: its q is read, its k | v are other data
    planes1 = [torch.randn(Z, nk, 3 * D, generator=g).to(dev).half() for _ in range(2)]      # image 1: its k | v are read
    for pl, src, col in ((planes0, qs * LOG2E, 0), (planes1, k, D), (planes1, v, 2 * D)):
        hi, lo = ops.split_f16(src.to(dev))
        pl[0][..., col:col + D] = hi
        pl[1][..., col:col + D] = lo
    oh = torch.empty(Z, nq, D, device=dev, dtype=torch.float16)
    ol = torch.empty_like(oh)
    st = torch.cuda.current_stream().cuda_stream
    eb = 2                                                                                   # bytes per plane element

    def call():
        rc = lib.og_attention(planes0[0].data_ptr(), planes0[1].data_ptr(), 3 * D,
                              planes1[0].data_ptr() + D * eb, planes1[1].data_ptr() + D * eb, 3 * D,
                              planes1[0].data_ptr() + 2 * D * eb, planes1[1].data_ptr() + 2 * D * eb, 3 * D,
                              oh.data_ptr(), ol.data_ptr(), D, Z, nq, nk, H, dh, None, st)
        _lib.check(rc, "og_attention")
    _, inst, _ = _traced(call)
    assert inst == {want}, (inst, want)
    o = ops.merge_f16(oh, ol).cpu()
    err = (o.double() - _ref(qs, k, v, H)[0]).abs().max().item()
    print(f"[dma addressing cross shape dh={dh} nq={nq} nk={nk} ld=3D] max |O - float64| {err:.2e}")
    assert torch.isfinite(o).all()
    assert err < TOL_O, err
