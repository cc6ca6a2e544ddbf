"""The weight-stationary q | k | v projection of 256-d batches (csrc/proj_wstat.hip: proj_wstat_kernel) through the stage entry
(ops.proj_block -> og_proj_block; planes as wide as the matrix, ranges of whole 256-column slabs, more than 8192 rows).

Every case asserts that proj_wstat_kernel is what ran (and that no other projection or GEMM kernel did), compares EVERY output element
with float64 of the unsplit inputs, and checks that nothing was written outside the requested ranges.  Shapes are the smallest that
reach the kernel (rows just above 8192) and that still meet every edge of its work split (csrc/og_proj_deal.h):

  block edges and dealing   8224 rows = 257 blocks over 255 workgroups (runs of 3 and 4 blocks); 8193 (the last block holds ONE row);
                            8192 + 32 x 255 + 7 (a partial last block behind whole ones)
  slab dealing              N = 512 / 768 / 1024 (teams of 2 / 3 / 4 workgroups), one slab in the middle of the matrix, k | v
  row split                 rows below the split take the q slab only, as the cross layer issues it; the split (block 125 of 375) is no
                            multiple of the runs (3 and 4 blocks)
  fewer units than workgroups   the rows below 8192 get NO slab, the 32 rows behind get three: 3 units, 253 workgroups exit at once
  stress magnitudes         x over 2^-6 .. 2^6 per element and a few weights of +-100 on top of 0.06 randn: the x_lo . w_hi and x_hi . w_lo
                            passes carry 2^-11 of every product, far above the bound
  byte equality             the planes equal, bit for bit, those of gemm_nt_f16x3_big2_kernel<2, 1> (the kernel these launches ran on
                            before) on the same operands

Tolerance: that of tests/test_gpu_parity.py test_proj_block_*: max(2 e32, 2e-6) + 2e-6 max|ref|, e32 = the error of the CPU fp32
evaluation of the same product against float64, measured in the case.  Every case prints err / bound."""
import functools
import os

import pytest
import torch

from openglue_amd import _lib, ops
from openglue_amd.kernel_trace import GEMM, PROJ_MLP, PROJ_WSTAT, launched_kernels
from tests.test_gpu_gemm_forms import _stop_after_a_gpu_fault  # noqa: F401  (autouse here too: nothing more runs on a device that faulted)

gpu = pytest.mark.gpu
K = 256


@pytest.fixture(scope="module", autouse=True)
def _threads():
    n = torch.get_num_threads()
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))      # float64 references beside the GPU
    yield
    torch.set_num_threads(n)
    _operands.cache_clear()


@functools.lru_cache(maxsize=2)
def _operands(M, N, stress=False):
    """x [M, K], w [N, K], bias [N] on the CPU, float64 x W^T + b and e32 of the same product in fp32.  Computed once per shape."""
    g = torch.Generator().manual_seed(4000 + M + N)
    x, w, b = torch.randn(M, K, generator=g) * 2.0, torch.randn(N, K, generator=g) * 0.06, torch.randn(N, generator=g) * 0.3
    if stress:
        x = torch.randn(M, K, generator=g) * torch.exp2(torch.rand(M, K, generator=g) * 12.0 - 6.0)
        idx = torch.randint(0, N * K, (64,), generator=g)
        w.view(-1)[idx] = torch.where(torch.rand(64, generator=g) < 0.5, -100.0, 100.0)       # 256 x 100 stays inside binary16
    ref = x.double() @ w.double().T + b.double()
    e32 = ((x @ w.T + b).double() - ref).abs().max().item()
    return x, w, b, ref, e32


def _case(gpu_device, M, N, split=0, cols_a=None, cols_b=None, stress=False):
    x, w, b, ref, e32 = _operands(M, N, stress)
    dev = lambda t: t.to(gpu_device)
    xd, wd, bd = dev(x), dev(w), dev(b)
    box = []
    names = launched_kernels(lambda: box.append(ops.proj_block(xd, wd, bd, split_row=split, cols_a=cols_a, cols_b=cols_b)))
    assert PROJ_WSTAT in names, names
    assert not [k for k in names if k.startswith(PROJ_MLP + GEMM)], names
    out = box[0].cpu()
    ca, cb = cols_a or (0, N), cols_b or (0, N)
    cut = 0 if split <= 0 else min(split, M)
    mask = torch.zeros(M, N, dtype=torch.bool)
    mask[:cut, ca[0]:ca[1]] = True
    mask[cut:, cb[0]:cb[1]] = True
    assert torch.isfinite(out).all()
    assert (out[~mask] == 0).all(), "written outside the requested ranges"
    err = ((out.double() - ref).abs() * mask).max().item()
    bound = max(2.0 * e32, 2e-6) + 2e-6 * ref.abs().max().item()
    print(f"[proj_wstat M={M} N={N} split={split} a={ca} b={cb} stress={stress}] err {err:.2e} bound {bound:.2e} (fp32 CPU err {e32:.2e})")
    assert err < bound, (err, bound)


@gpu
@pytest.mark.parametrize("M", [8224, 8193, 8192 + 32 * 255 + 7])
def test_block_edges_and_dealing(gpu_device, M):
    _case(gpu_device, M, 768)


@gpu
@pytest.mark.parametrize("N,cols_b", [(512, None), (768, None), (1024, None), (768, (256, 512)), (768, (256, 768))])
def test_slab_dealing(gpu_device, N, cols_b):
    _case(gpu_device, 8224, N, cols_b=cols_b)


@gpu
def test_row_split(gpu_device):
    """125 blocks x 1 slab + 250 blocks x 3 slabs: og_proj_deal gives range A 32 workgroups and range B 74 teams of 3, runs of 3 and 4
    blocks in both: the split at block 125 is no multiple of either."""
    _case(gpu_device, 12000, 768, split=4000, cols_a=(0, 256), cols_b=(0, 768))


@gpu
def test_fewer_units_than_workgroups(gpu_device):
    _case(gpu_device, 8224, 768, split=8192, cols_a=(0, 0), cols_b=(0, 768))


@gpu
def test_stress_magnitudes(gpu_device):
    _case(gpu_device, 8224, 768, stress=True)


@gpu
def test_planes_bit_identical_to_the_tile_gemm(gpu_device):
    """16384 x 768: 64 x 3 = 192 tiles, the fewest the launcher gives gemm_nt_f16x3_big2_kernel<2, 1>."""
    M, N = 16384, 768
    x, w, b, _, _ = _operands(M, N)
    dev = gpu_device
    rows = ops.split_f16_hl(x.to(dev))
    bias = b.to(dev)
    inv = torch.full((1,), 1.0 / 256.0, device=dev)
    lib = _lib.load()
    st = torch.empty(lib.og_proj_block_stream_bytes(N, K), dtype=torch.uint8)
    _lib.check(lib.og_proj_block_pack(N, K, w.data_ptr(), st.data_ptr()), "og_proj_block_pack")
    st = st.to(dev)
    planes = lambda: [torch.zeros(M, N, device=dev, dtype=torch.float16) for _ in range(2)]
    (yh, yl), (zh, zl) = planes(), planes()
    names = launched_kernels(lambda: _lib.call("og_proj_block", dev, rows.data_ptr(), 2 * K, M, K, N, st.data_ptr(), bias.data_ptr(), inv.data_ptr(),
                                               yh.data_ptr(), yl.data_ptr(), N, 0, 0, 0, 0, N // 32, _lib.STREAM))
    assert names == [PROJ_WSTAT], names
    w_hl = ops.split_f16_hl((w * 256.0).to(dev))
    names = launched_kernels(lambda: _lib.call("og_gemm_nt_f16x3", dev, rows.data_ptr(), 2 * K, w_hl.data_ptr(), 2 * K, M, N, K, 1.0 / 256.0, bias.data_ptr(), 0,
                                               None, N, None, N, zh.data_ptr(), zl.data_ptr(), N, 0, _lib.STREAM))
    assert names == ["gemm_nt_f16x3_big2_kernel<2, 1>"], names
    I16 = torch.int16
    assert torch.equal(yh.view(I16), zh.view(I16)) and torch.equal(yl.view(I16), zl.view(I16))
    assert yh.abs().max().item() > 0
