"""The widened store tail of the attention forward kernels (og_attn_store_o, csrc/attention.hip) at the smallest shapes where it can go wrong.

The tail swaps the packed (hi, lo) output dwords of each pair of 8-channel slots between the half-waves (v_permlane32_swap) and stores one
16-byte run per pair and plane; an `ldo` that is no multiple of 8 halves keeps the 8-byte stores.  What can go wrong: the operand order of the
swap or the upper half-wave's column (a wrong image inside a query row), a lane that skips the swap (partial 32-query blocks), the plane / hl32
column mapping, and the guard of the padded dh = 16 block.  The cases:

  a. planes through ops.attention against float64 softmax attention: Z = 2, (H, dh) in (4, 16), (4, 32), (4, 64), (2, 128), query counts
     {1, 31, 33, 129} (partial 32-query blocks that end in either half of a 128-query tile, and a partial second tile) x key counts {1, 65}
     (a one-tile problem, whose tile 0 is also the masked last tile, and a two-tile one), and the key split once;
  b. gap columns through lib.og_attention: ldo = D + 64 (16-byte stores) and ldo = D + 4 (8-byte stores) with a sentinel in the output's gap
     and NaN in the inputs' gaps: the sentinel stays, O is bit-identical to the compact call;
  c. the hl32 output layout, which og_forward writes, through SuperGlue.match against the float64 oracle at one pair of 129 x 129 and of
     33 x 65 keypoints (256-d) and 129 x 129 (128-d).  (At these sizes the dispatch picks the plain form; the grid-split forms, whose merge
     stands in front of the same tail, run at their own sizes in tests/test_gpu_attention_dispatch.py.)

Every case asserts the attention instances it launched (tests/test_gpu_attention_dispatch.py's restatement of the dispatch rule).
"""
import pytest
import torch

from openglue_amd import _lib, ops, synthetic as syn
from tests.test_gpu_attention_dispatch import KS64, _ref, _traced, expected_instance, forward_instances
from tests.test_gpu_attention_dma_addressing import TOL_O
from tests.test_gpu_parity import TOL_SCORES, _build, _index_agreement
from tests.util import MATCH_THRESHOLD, to_device

pytestmark = pytest.mark.gpu

LOG2E = 1.4426950408889634
HEADS = ((4, 16), (4, 32), (4, 64), (2, 128))
NQS = (1, 31, 33, 129)
NKS = (1, 65)


def _inputs(Z, nq, nk, H, dh, seed):
    g = torch.Generator().manual_seed(seed)
    D = H * dh
    q, k, v = torch.randn(Z, nq, D, generator=g) * 3.0, torch.randn(Z, nk, D, generator=g) * 3.0, torch.randn(Z, nk, D, generator=g) * 2.0
    return q * dh ** -0.5, k, v


@pytest.fixture(scope="module")
def plane_references():
    """inputs and float64 results of the whole matrix, computed once"""
    out = {}
    for H, dh in HEADS:
        for nq in NQS:
            for nk in NKS:
                qs, k, v = _inputs(2, nq, nk, H, dh, nq * 7919 + nk * 31 + dh)
                out[dh, nq, nk] = (qs, k, v, _ref(qs, k, v, H)[0])
    return out


def _check_planes(dev, tag, qs, k, v, O, H, want):
    o, inst, _ = _traced(lambda: ops.attention(qs.to(dev), k.to(dev), v.to(dev), H))
    assert inst == {want}, (inst, want)
    o = o.cpu()
    err = (o.double() - O).abs().max().item()
    print(f"[store tail {tag}] {want}: max |O - float64| {err:.2e} (bound {TOL_O:.1e})")
    assert torch.isfinite(o).all(), tag
    assert err < TOL_O, (tag, err)


@pytest.mark.parametrize("H,dh", HEADS)
@pytest.mark.parametrize("nk", NKS)
def test_planes_against_float64(gpu_device, plane_references, H, dh, nk):
    want = f"attention_dma_kernel<{dh}, RaggedNone, 1, 1, 0, 0>" if dh in (32, 64) else f"attention_kernel<{dh}, RaggedNone>"
    for nq in NQS:
        assert expected_instance(2, H, dh, nq, nk) == want
        qs, k, v, O = plane_references[dh, nq, nk]
        _check_planes(gpu_device, f"dh={dh} nq={nq} nk={nk}", qs, k, v, O, H, want)


def test_planes_key_split(gpu_device):
    H, dh, nq, nk = 4, 64, 129, 257
    assert expected_instance(2, H, dh, nq, nk) == KS64
    qs, k, v = _inputs(2, nq, nk, H, dh, 41)
    _check_planes(gpu_device, f"key split nq={nq} nk={nk}", qs, k, v, _ref(qs, k, v, H)[0], H, KS64)


@pytest.mark.parametrize("dh", [64, 32])
def test_gap_columns_wide_and_narrow_stores(gpu_device, dh):
    """ldo = D + 64: a multiple of 8 halves, the 16-byte stores; ldo = D + 4: the 8-byte stores.  Both leave the gap alone and equal the compact call bit for bit."""
    lib = _lib.load()
    Z, H, nq, nk = 2, 4, 129, 65
    D = H * dh
    dev = gpu_device
    g = torch.Generator().manual_seed(dh + 3)
    q = (torch.randn(Z, nq, D, generator=g) * 3.0 * dh ** -0.5 * LOG2E).to(dev)
    k, v = (torch.randn(Z, nk, D, generator=g) * 3.0).to(dev), (torch.randn(Z, nk, D, generator=g) * 2.0).to(dev)
    planes = [p for t in (q, k, v) for p in ops.split_f16(t)]
    st = torch.cuda.current_stream().cuda_stream
    want = expected_instance(Z, H, dh, nq, nk)
    assert want == f"attention_dma_kernel<{dh}, RaggedNone, 1, 1, 0, 0>"

    def call(ins, outs, ld_in, ld_out):
        qh, ql, kh, kl, vh, vl = ins
        rc = lib.og_attention(qh.data_ptr(), ql.data_ptr(), ld_in, kh.data_ptr(), kl.data_ptr(), ld_in, vh.data_ptr(), vl.data_ptr(), ld_in,
                              outs[0].data_ptr(), outs[1].data_ptr(), ld_out, Z, nq, nk, H, dh, None, st)
        _lib.check(rc, "og_attention")

    compact = [torch.empty(Z, nq, D, device=dev, dtype=torch.float16) for _ in range(2)]
    _, inst, _ = _traced(lambda: call(planes, compact, D, D))
    assert inst == {want}, (inst, want)
    ref, _ = _ref(q.cpu() / LOG2E, k.cpu(), v.cpu(), H)
    err = (ops.merge_f16(*compact).cpu().double() - ref).abs().max().item()
    print(f"[store tail gap columns dh={dh}] compact: max |O - float64| {err:.2e} (bound {TOL_O:.1e})")
    assert err < TOL_O, err
    ld_in = D + 64
    wide = []
    for p in planes:
        w = torch.full((*p.shape[:2], ld_in), float("nan"), device=dev, dtype=torch.float16)
        w[..., :D] = p
        wide.append(w)
    sentinel = 12344.0
    for ldo in (D + 64, D + 4):
        # rows of the D + 4 buffer start at 8-byte, not 16-byte, multiples: the case the 8-byte stores are kept for
        owide = [torch.full((Z, nq, ldo), sentinel, device=dev, dtype=torch.float16) for _ in range(2)]
        _, inst2, _ = _traced(lambda: call(wide, owide, ld_in, ldo))
        assert inst2 == {want}, (inst2, want)
        for c, w in zip(compact, owide):
            assert torch.equal(w[..., :D], c), ldo
            assert (w[..., D:] == sentinel).all(), ldo


@pytest.mark.parametrize("D,m,n", [(256, 129, 129), (256, 33, 65), (128, 129, 129)])
def test_hl32_layout_through_forward(gpu_device, D, m, n):
    """og_forward writes O in the hl32 layout: hi columns of a 32-channel group, then its lo columns"""
    H, B = 4, 1
    cfg = syn.make_config(descriptor_dim=D, num_stages=2, num_heads=H, num_iters=20, side_info_size=1)
    sd = syn.make_state_dict(cfg, seed=0)
    model = _build(cfg, sd, gpu_device)
    data = syn.make_batch(B, m, n, D, 1, seed=23)
    dd = to_device(data, gpu_device)
    out, inst, _ = _traced(lambda: model.match(dd, MATCH_THRESHOLD))
    want = forward_instances(B, m, n, H, D // H)
    assert inst == want, (inst, want)
    out = {k: v.cpu() for k, v in out.items()}
    ndiff, unexplained, o64 = _index_agreement(out["matches0"], out["scores"], sd, cfg, data)
    err = (out["scores"].double() - o64["scores"]).abs().max().item()
    print(f"[store tail forward D={D} {m}x{n}] {sorted(want)}: scores err {err:.2e} (bound {TOL_SCORES:.1e}) exempt={ndiff}")
    assert torch.isfinite(out["scores"]).all()
    assert err < TOL_SCORES, err
    assert unexplained == 0, (ndiff, unexplained)
