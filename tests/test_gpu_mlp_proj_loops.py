"""The batch message MLP (csrc/mlp_fused.hip: mlp_fused_kernel) and the weight-stationary q | k | v projection (csrc/proj_wstat.hip:
proj_wstat_kernel) after their loops lost the bookkeeping: peeled last stages / blocks, compile-time ring slots, scalar DMA and store bases,
the residual's identity fragment in LDS, the clamp and the row predicate only where a tile can be partial.

MLP, through ops.mlp_block (asserting that mlp_fused_kernel<D> ran):
  D = 256 at M = 8193 (the first row count that takes the batch kernel; the last tile holds ONE row), 8320 (whole tiles), 8447 (a 127-row
  tail); D = 128 at M = 8193.  Against float64 on the first and last rows at the tolerance of tests/test_gpu_parity.py
  test_mlp_block_fused_vs_float64: max(2 e32, 2e-6) + 2e-6 max|ref|, e32 = the error of the CPU fp32 evaluation.  And BITWISE: rows [0, M)
  of the M-row call equal the same rows of a call on the input padded with OTHER data to the next multiple of 128 rows -- a tile's result
  does not depend on what lies behind row M - 1 (clamped loads, predicated stores, the peeled stages).

Projection, through og_proj_block (asserting that proj_wstat_kernel ran and nothing else): the smallest row counts that reach the kernel
(og_proj_plan.h: more than 8192 rows) -- 8224, 8193, 8223, i.e. M % 32 = 0, 1, 31, all 257 blocks -- as a 3-slab launch (85 teams: runs
of 3 and 4 blocks), a 2-slab launch (k | v; 128 teams: runs of 2 and 3) and a row-split launch (q for the rows below 2720, q | k | v for the
others); a port of og_proj_deal (csrc/og_proj_deal.h) asserts that runs of odd AND even length occur in every case.  Those runs end inside
the generic first / last blocks of the kernel, so one more 3-slab case, 24481 rows (766 blocks: runs of 9 and 10), goes through the steady
loop.  Every case is bit-identical, on the requested ranges, to gemm_nt_f16x3_big2_kernel<2, 1> on the same operands (the rows padded
with zeros to 16384 or more so that the launcher picks that kernel), exactly as tests/test_gpu_proj_wstat.py compares them; nothing is
written outside the ranges."""
import functools
import os

import pytest
import torch

from openglue_amd import _lib, ops
from openglue_amd.kernel_trace import PROJ_WSTAT, launched_kernels, proj_mlp_instances
from tests.test_gpu_gemm_forms import _stop_after_a_gpu_fault  # noqa: F401  (autouse here too: nothing more runs on a device that faulted)

gpu = pytest.mark.gpu
I16 = torch.int16


@pytest.fixture(scope="module", autouse=True)
def _threads():
    n = torch.get_num_threads()
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))      # float64 references beside the GPU
    yield
    torch.set_num_threads(n)
    _proj_reference.cache_clear()


# ------------------------------------------------------------------ message MLP ------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("D,M", [(256, 8193), (256, 8320), (256, 8447), (128, 8193)])
def test_mlp_tail_rows_and_float64(gpu_device, D, M):
    g = torch.Generator().manual_seed(7000 + M + D)
    Mp = (M + 127) // 128 * 128
    rnd = lambda *s, scale: torch.randn(*s, generator=g) * scale
    x, o = rnd(Mp, D, scale=2.0), rnd(Mp, D, scale=1.5)            # rows [M, Mp): the OTHER data of the padded call
    w0, w3, b0, b3 = rnd(2 * D, 2 * D, scale=0.04), rnd(D, 2 * D, scale=0.05), rnd(2 * D, scale=0.3), rnd(D, scale=0.3)
    dev = lambda t: t.to(gpu_device)
    wd = [dev(t) for t in (w0, b0, w3, b3)]
    box = []
    names = launched_kernels(lambda: box.append(ops.mlp_block(dev(x[:M].contiguous()), dev(o[:M].contiguous()), *wd)))
    assert proj_mlp_instances(names) == [f"mlp_fused_kernel<{D}>"], names
    out = box[0].cpu()
    if Mp > M:
        names = launched_kernels(lambda: box.append(ops.mlp_block(dev(x), dev(o), *wd)))
        assert proj_mlp_instances(names) == [f"mlp_fused_kernel<{D}>"], names
        padded = box[1].cpu()
        assert torch.equal(out.view(torch.int32), padded[:M].view(torch.int32)), "rows [0, M) depend on what lies behind them"
    xo_in = ops.merge_f16_hl(ops.split_f16_hl(dev(torch.cat([x[:M], o[:M]], 1).contiguous()))).cpu()       # what the kernel is given
    sl = torch.cat([torch.arange(0, 256), torch.arange(M - 384, M)])
    ref = xo_in[sl, :D].double() + torch.relu(xo_in[sl].double() @ w0.double().T + b0.double()) @ w3.double().T + b3.double()
    e32 = ((xo_in[sl, :D] + torch.relu(xo_in[sl] @ w0.T + b0) @ w3.T + b3).double() - ref).abs().max().item()
    err = (out[sl].double() - ref).abs().max().item()
    bound = max(2.0 * e32, 2e-6) + 2e-6 * ref.abs().max().item()
    print(f"[mlp loops D={D} M={M}] err {err:.2e} bound {bound:.2e} (fp32 CPU err {e32:.2e})")
    assert torch.isfinite(out).all()
    assert err < bound, (err, bound)


# ------------------------------------------------------------------ projection -------------------------------------------------------------------
K, N, G = 256, 768, 256


def _run_lengths(M, split, na, nb):
    """csrc/og_proj_deal.h, og_proj_deal_rows + og_proj_deal_unit: the lengths (in 32-token blocks) of the runs the workgroups walk."""
    blocks = (M + 31) // 32
    ba = 0 if split <= 0 else blocks if split >= M else split // 32
    bb = blocks - ba
    if ba <= 0 or na <= 0:
        ba = na = 0
    if bb <= 0 or nb <= 0:
        bb = nb = 0
    ta = tb = 0
    if ba and not bb:
        ta = min(G // na, ba)
    elif bb and not ba:
        tb = min(G // nb, bb)
    elif ba and bb:
        best, t = 1 << 30, 1
        while t * na < G and t <= ba:
            u = min((G - t * na) // nb, bb)
            if u < 1:
                break
            longest = max(-(-ba // t), -(-bb // u))
            if longest < best:
                best, ta, tb = longest, t, u
            t += 1
    runs = [(i + 1) * ba // ta - i * ba // ta for i in range(ta)] + [(i + 1) * bb // tb - i * bb // tb for i in range(tb)]
    return [r for r in runs if r > 0]


@functools.lru_cache(maxsize=4)
def _proj_reference(M, device):
    """Operands of an M-row case and the planes of gemm_nt_f16x3_big2_kernel<2, 1> for all N columns (computed once per M)."""
    g = torch.Generator().manual_seed(8000 + M)
    x, w, b = torch.randn(M, K, generator=g) * 2.0, torch.randn(N, K, generator=g) * 0.06, torch.randn(N, generator=g) * 0.3
    Mr = max(16384, (M + 255) // 256 * 256)
    xr = torch.zeros(Mr, K)
    xr[:M] = x
    rows = ops.split_f16_hl(xr.to(device))
    bias = b.to(device)
    lib = _lib.load()
    st = torch.empty(lib.og_proj_block_stream_bytes(N, K), dtype=torch.uint8)
    _lib.check(lib.og_proj_block_pack(N, K, w.data_ptr(), st.data_ptr()), "og_proj_block_pack")
    st = st.to(device)
    w_hl = ops.split_f16_hl((w * 256.0).to(device))
    zh, zl = (torch.zeros(Mr, N, device=device, dtype=torch.float16) for _ in range(2))
    names = launched_kernels(lambda: _lib.call("og_gemm_nt_f16x3", device, rows.data_ptr(), 2 * K, w_hl.data_ptr(), 2 * K, Mr, N, K, 1.0 / 256.0, bias.data_ptr(), 0,
                                               None, N, None, N, zh.data_ptr(), zl.data_ptr(), N, 0, _lib.STREAM))
    assert names == ["gemm_nt_f16x3_big2_kernel<2, 1>"], names
    return rows, st, bias, zh[:M].cpu(), zl[:M].cpu()


FORMS = {"three_slabs": (0, (0, 0), (0, 768)), "two_slabs": (0, (0, 0), (256, 768)), "row_split": (2720, (0, 256), (0, 768))}


@gpu
@pytest.mark.parametrize("form,M", [(f, m) for f in FORMS for m in (8224, 8193, 8223)] + [("three_slabs", 24481)])
def test_proj_wstat_bit_identical_to_the_tile_gemm(gpu_device, form, M):
    split, ca, cb = FORMS[form]
    runs = _run_lengths(M, split, (ca[1] - ca[0]) // 256, (cb[1] - cb[0]) // 256)
    assert any(r & 1 for r in runs) and any(not r & 1 for r in runs), runs
    if M == 24481:
        assert min(runs) >= 8, runs                                   # at least one iteration of the steady loop in every workgroup
    rows, st, bias, zh, zl = _proj_reference(M, gpu_device)
    dev = gpu_device
    inv = torch.full((1,), 1.0 / 256.0, device=dev)
    yh, yl = (torch.zeros(M, N, device=dev, dtype=torch.float16) for _ in range(2))
    names = launched_kernels(lambda: _lib.call("og_proj_block", dev, rows.data_ptr(), 2 * K, M, K, N, st.data_ptr(), bias.data_ptr(), inv.data_ptr(),
                                               yh.data_ptr(), yl.data_ptr(), N, split, ca[0] // 32, ca[1] // 32, cb[0] // 32, cb[1] // 32, _lib.STREAM))
    assert names == [PROJ_WSTAT], names
    mask = torch.zeros(M, N, dtype=torch.bool)
    mask[:split, ca[0]:ca[1]] = True
    mask[split:, cb[0]:cb[1]] = True
    yh, yl = yh.cpu(), yl.cpu()
    print(f"[proj loops {form} M={M}] runs of {sorted(set(runs))} blocks")
    for y, z in ((yh, zh), (yl, zl)):
        assert (y.view(I16)[~mask] == 0).all(), "written outside the requested ranges"
        assert torch.equal(y.view(I16)[mask], z.view(I16)[mask])
    assert yh.abs().max().item() > 0
