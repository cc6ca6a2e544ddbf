"""Every q | k | v projection and message-MLP form the default dispatch launches (csrc/mlp_fused.hip), pinned to float64 on EVERY output
element, with the launched instance asserted.

og_launch_mlp_fused and the projection plan (csrc/og_proj_plan.h, under og_proj_block's and og_forward's policy) pick the kernel from the row
count, the alignment of the biases, the column ranges, the leading dimension and alignment of the output planes and the row split.
tests/proj_plan_ref.py restates those rules (from the call sites as they stood before the plan header; tests/test_proj_plan_cpu.py holds the
header to it); every GPU case asserts that the launches it made are exactly the predicted ones, so a case cannot drift onto another kernel
unnoticed.  `parts` / `bpp` (how proj_small_kernel's launch deals the output blocks of a token tile out to workgroups) and the per-wave
block count cannot be observed from the kernel name: their restatement (`proj_small_grid`, `wave_blocks`, section 0) is there to prove
that each shape sits on the intended side of a threshold, and the case ids carry what it predicts.

  0. the restatement itself, on both sides of every boundary (CPU)
  1. the message MLP through _lib (og_mlp_block_pack, og_mlp_block), D = 256 / 128: rows of ld = 4D + 8 halves with NaN in the gap of every
     row and in the rows past M; the whole x half against float64, the O half, the gaps and the rows past M bit-identical to before.
     mlp_small_kernel by size, mlp_fused_kernel by size (from M = 8193) and by a bias that is not 16-byte aligned (M = 1 .. 200, where
     nothing else runs the 128-token kernel), the launcher's refusals
  2. the projections through _lib (og_proj_block_pack, og_proj_block), K = 256 / 128: X as [x | O] rows of 4K halves with NaN in the O half
     and in the rows past M, planes of ldy > N halves in a sentinel with rows past M.  proj_small_kernel: every per-wave block count, both
     sides of the deal-out rule, ranges that start in the middle of the matrix, the row split (also with an empty range and with
     split_row >= M), the forced deal-out with a ragged last part.  proj_stream_kernel: partial last tiles, every group position, the row
     split, the widest range it takes.  The fall-backs of the stage entry to proj_small_kernel above 8192 rows, the refusals
  3. the forms og_forward launches, through SuperGlue (one stage): EVERY projection and message-MLP launch of one traced call, in launch
     order -- the kernels of mlp_fused.hip, proj_wstat_kernel and the tile GEMMs a projection falls to -- against the restatement, x at tap 1 against the float64 oracle's self layer applied to tap 0, x at tap 2 against its cross layer applied to
     tap 1.  One case gives the three split-f16 matrices of each layer three DIFFERENT power-of-two pre-scales (read back from the packed
     blob and asserted pairwise different first): the only place MlpFusedArgs::scales_dev is pinned at a layer

Tolerance (sections 1, 2): e32 = the max error of the CPU fp32 evaluation of the same operands against float64, measured in the case;
the bound is max(2 e32, 2e-6) + 2e-6 max|ref| (tests/test_gpu_parity.py: test_mlp_block_fused_vs_float64, test_proj_block_*), on the whole
output.  The reference is float64 on merge(split(.)) of every operand, what the kernel is given.  Every case prints err / bound.
Section 3: TOL_TAP x scale (tests/test_gpu_parity.py: test_stage_taps_against_reference_layers).

instance -> a case that asserts it
  mlp_small_kernel<256>     test_mlp_small[256-*], test_mlp_unaligned_bias_takes_the_tile_kernel[256-*] (aligned twin), test_forward_forms[d256-*]
  mlp_small_kernel<128>     test_mlp_small[128-*], test_mlp_unaligned_bias_takes_the_tile_kernel[128-*] (aligned twin), test_forward_forms[d128-*]
  mlp_fused_kernel<256>     test_mlp_fused_by_size[256-*], test_mlp_unaligned_bias_takes_the_tile_kernel[256-*], test_forward_forms[d256-B2-m128-n4100]
  mlp_fused_kernel<128>     test_mlp_fused_by_size[128-*], test_mlp_unaligned_bias_takes_the_tile_kernel[128-*], test_forward_forms[d128-*]
  proj_small_kernel<256>    test_proj_small_full[256-*], test_proj_small_ranges[K256-*], test_proj_small_row_split[256-*], test_proj_fall_backs[256-*]
  proj_small_kernel<128>    test_proj_small_full[128-*], test_proj_small_ranges[K128-*], test_proj_small_row_split[128-*], test_proj_fall_backs[128-*]
  proj_stream_kernel<256>   test_proj_stream_full[256-*], test_proj_stream_groups[256-*], test_proj_stream_row_split[256-*], test_proj_stream_widest[256]
  proj_stream_kernel<128>   test_proj_stream_full[128-*], test_proj_stream_groups[128-*], test_proj_stream_row_split[128-*], test_forward_forms[d128-*]
  proj_wstat_kernel         test_forward_forms[d256-B12-*] (a self launch), [d256-B16-*] (self, the row split, k | v); tests/test_gpu_proj_wstat.py pins its values
not covered, and why:
  OG_PROJ_PARTS=0                           one workgroup per token tile whatever the shape: an experiment knob, read once per process
  OG_PROJ_STREAM, OG_PROJ_SMALL             forced kernel choices (experiments, read once per process): which launches they move is checked
                                            without a GPU (tests/test_proj_plan_cpu.py); the kernels they move them to are pinned here
  OG_MLP_FUSED=0, OG_MLP_SMALL              fc.0 / fc.3 as two GEMM launches, a forced kernel choice: experiments; the GEMM forms are
                                            pinned in tests/test_gpu_gemm_forms.py
  proj_stream_kernel<256> under og_forward  og_forward packs the batch stream at D = 128 only (api.hip: packed_layout); the K = 256 form
                                            is reachable through the stage entry alone (section 2)
  proj_small_kernel without the row clamp   the rows past M of a partial tile are other TOKENS (columns of the MFMA's B operand): what is
                                            loaded for them never reaches a stored element, so the clamp `r > g.M - 1` guards the
                                            address only and no value check can see it.  NaN rows past M are there for the leading
                                            dimension and the O half, which do reach stored elements
"""
import functools
import os

import pytest
import torch

from openglue_amd import _lib, ops, synthetic as syn
from openglue_amd.kernel_trace import launched_kernels, proj_mlp_instances, projection_candidates
from oracle import superglue_oracle as orc
from tests.test_gpu_gemm_forms import NAN, SENT, TOL_TAP, _dev, _stop_after_a_gpu_fault  # noqa: F401  (the fixture is autouse here too)
from tests.proj_plan_ref import expected_forward, expected_mlp, expected_proj_block, forward_sequence
from tests.util import to_device

# The dispatch knobs are read once per process: one left in the environment would move every case below to another kernel.
_KNOBS = sorted(k for k in os.environ if k.startswith(("OG_MLP_", "OG_PROJ_")))
if _KNOBS:
    raise RuntimeError(f"test_gpu_proj_mlp_forms runs the default dispatch: unset {_KNOBS}")

OG_E_INVALID, OG_E_SHAPE, OG_E_ALIGN = -1, -2, -3          # include/openglue_amd.h


def _cdiv(a, b):
    return (a + b - 1) // b


# ----------------------------------------------------------------------------- 0. the selection rules, restated
def proj_small_grid(M, a, b):
    """launch_proj_small (mlp_fused.hip) -> (parts, bpp, workgroups)."""
    tiles, nblk = _cdiv(M, 32), max(a[1] - a[0], b[1] - b[0])
    parts, bpp = 1, max(nblk, 1)
    if nblk > 8 and tiles * _cdiv(nblk, 8) <= 256:         # few tiles: 8 blocks (one per wave) per workgroup
        parts, bpp = _cdiv(nblk, 8), 8
    if nblk > 24:                                          # a workgroup covers at most 3 blocks per wave
        parts, bpp = _cdiv(nblk, 8), 8
    return parts, bpp, tiles * parts


def wave_blocks(n):
    """proj_small_kernel (mlp_fused.hip:1336): how many of the n blocks of a workgroup each of its eight waves owns."""
    return [(n - w + 7) // 8 for w in range(8)]


def proj_small_forms(M, a, b, split_row=0):
    """The proj_small_run<NB> instantiations a launch reaches (0 = an idle wave), from the grid rule and the per-wave count."""
    parts, bpp, _ = proj_small_grid(M, a, b)
    ranges = [b] if split_row <= 0 else [a] if split_row >= M else [a, b]
    nb = set()
    for r0, r1 in ranges:
        for p in range(parts):
            cb0 = r0 + p * bpp
            cb1 = min(cb0 + bpp, r1)
            if cb1 > cb0:
                nb |= {min(v, 3) for v in wave_blocks(cb1 - cb0)}
    return parts, bpp, sorted(nb)


def test_restatement_sides_of_the_boundaries():
    """The boundaries of the launchers and of og_forward's routing as the restatement sees them (a wrong restatement would make every
    assertion below pointless)."""
    for D in (256, 128):
        ms, mf, ps, pst = (f"{k}<{D}>" for k in ("mlp_small_kernel", "mlp_fused_kernel", "proj_small_kernel", "proj_stream_kernel"))
        assert expected_mlp(8192, D) == ms and expected_mlp(8193, D) == mf
        assert expected_mlp(200, D, b0_aligned=False) == mf and expected_mlp(200, D, b3_aligned=False) == mf and expected_mlp(200, D) == ms
        # the stage entry: 8192 / 8193 rows, N = 1024 (8 groups) / 1152 (9), ldy, a ragged range, the split row, the plane alignment
        full = lambda N: ((0, 0), (0, N // 32))
        assert expected_proj_block(8192, D, 3 * D, *full(3 * D), 3 * D + 64) == ps
        assert expected_proj_block(8193, D, 3 * D, *full(3 * D), 3 * D + 64) == pst
        assert expected_proj_block(8193, D, 1024, *full(1024), 1024 + 64) == pst
        assert expected_proj_block(8193, D, 1152, *full(1152), 1152 + 64) == ps
        assert expected_proj_block(8193, D, 3 * D, *full(3 * D), 3 * D + 4) == ps
        assert expected_proj_block(8193, D, 3 * D, (0, 0), (0, 3 * D // 32 - 2), 3 * D + 64) == ps
        assert expected_proj_block(8193, D, 3 * D + 32, *full(3 * D + 32), 3 * D + 96) == ps                    # N % 128 != 0
        assert expected_proj_block(8320, D, 3 * D, (0, D // 32), (0, 3 * D // 32), 3 * D + 64, split_row=8192) == pst
        assert expected_proj_block(8320, D, 3 * D, (0, D // 32), (0, 3 * D // 32), 3 * D + 64, split_row=8224) == ps
        assert expected_proj_block(8320, D, 3 * D, (0, D // 32), (0, 3 * D // 32), 3 * D + 64, split_row=8320) == pst    # split_row >= M
        assert expected_proj_block(8193, D, 3 * D, *full(3 * D), 3 * D + 64, planes_aligned=False) == ps
    # launch_proj_small: tiles * parts <= 256 at 24 blocks (3 parts) and at 12 (2 parts); 8 / 9 blocks; 24 / 25 blocks
    assert proj_small_grid(2720, (0, 0), (0, 24)) == (3, 8, 255) and proj_small_grid(2721, (0, 0), (0, 24)) == (1, 24, 86)
    assert proj_small_grid(4096, (0, 0), (0, 12)) == (2, 8, 256) and proj_small_grid(4097, (0, 0), (0, 12)) == (1, 12, 129)
    assert proj_small_grid(96, (0, 0), (0, 8)) == (1, 8, 3) and proj_small_grid(96, (0, 0), (0, 9)) == (2, 8, 6)
    assert proj_small_grid(2752, (0, 0), (5, 29)) == (1, 24, 86) and proj_small_grid(2752, (0, 0), (5, 30)) == (4, 8, 344)
    assert proj_small_grid(100, (0, 0), (0, 32)) == (4, 8, 16) and proj_small_grid(100, (0, 0), (0, 36)) == (5, 8, 20)
    assert proj_small_grid(96, (0, 8), (0, 24)) == (3, 8, 9) and proj_small_grid(4128, (0, 8), (0, 24)) == (1, 24, 129)    # the wider range counts
    assert proj_small_grid(96, (3, 3), (0, 0)) == (1, 1, 3)
    # the per-wave count: 20 blocks = waves 0-3 three, 4-7 two; 1 .. 7 blocks leave waves idle
    assert wave_blocks(24) == [3] * 8 and wave_blocks(20) == [3] * 4 + [2] * 4 and wave_blocks(12) == [2] * 4 + [1] * 4
    assert wave_blocks(8) == [1] * 8 and wave_blocks(7) == [1] * 7 + [0] and wave_blocks(1) == [1] + [0] * 7 and wave_blocks(23) == [3] * 7 + [2]
    assert proj_small_forms(2752, (0, 0), (5, 25)) == (1, 20, [2, 3]) and proj_small_forms(96, (0, 0), (5, 25)) == (3, 8, [0, 1])
    assert proj_small_forms(100, (0, 0), (0, 36)) == (5, 8, [0, 1])                      # the last part: 4 blocks, waves 4-7 idle
    assert proj_small_forms(4128, (0, 8), (0, 24), split_row=32) == (1, 24, [1, 3])      # not dealt out: rows of image 0 one block per wave
    # og_forward: T0 % 32 and T0 % 128 zero and non-zero, T = 8192 / 8193 at both widths
    k = lambda D: tuple(f"{n}<{D}>" for n in ("mlp_small_kernel", "mlp_fused_kernel", "proj_small_kernel", "proj_stream_kernel"))
    ms, mf, ps, pst = k(256)
    assert expected_forward(256, 1, 128, 160) == {ps: 3, ms: 3}                          # T0 % 32 == 0: one launch with a row split
    assert expected_forward(256, 1, 130, 97) == {ps: 4, ms: 3}                           # three launches in the cross layer
    assert expected_forward(256, 2, 128, 4100) == {ps: 2, ms: 1, mf: 2}                  # T = 8456: the big launches are GEMMs
    assert expected_forward(256, 1, 128, 8064) == {ps: 3, ms: 3}                         # T = 8192
    assert expected_forward(256, 1, 128, 8065) == {ps: 3, ms: 2, mf: 1}                  # T = 8193: image 1 alone is 8065 rows
    assert expected_forward(256, 2, 256, 32512) == {ps: 1, ms: 1, mf: 2}                 # 2 + 254 x 3 = 764 blocks: the GEMM row split
    ms, mf, ps, pst = k(128)
    assert expected_forward(128, 2, 128, 4100) == {pst: 2, ps: 1, mf: 2, ms: 1}          # T0 % 128 == 0: the stream launch with a row split
    assert expected_forward(128, 2, 130, 4100) == {pst: 2, ps: 2, mf: 2, ms: 1}          # T0 = 260: a stream launch at row offset T0
    assert expected_forward(128, 1, 128, 8064) == {ps: 3, ms: 3}                         # T = 8192
    assert expected_forward(128, 1, 128, 8065) == {pst: 2, ps: 1, mf: 1, ms: 2}          # T = 8193
    assert expected_forward(128, 1, 128, 160) == {ps: 3, ms: 3} and expected_forward(128, 1, 130, 97) == {ps: 4, ms: 3}
    # the stage entry reaches proj_wstat_kernel where the planes are as wide as the matrix: 8192 / 8193 rows, ldy, a range of whole slabs or not
    assert expected_proj_block(8193, 256, 768, *full(768), 768) == "proj_wstat_kernel" and expected_proj_block(8192, 256, 768, *full(768), 768) == "proj_small_kernel<256>"
    assert expected_proj_block(8193, 256, 768, *full(768), 768 + 64) == "proj_stream_kernel<256>" and expected_proj_block(8193, 128, 384, *full(384), 384) == "proj_stream_kernel<128>"
    assert expected_proj_block(8193, 256, 768, (0, 0), (4, 24), 768) == "proj_stream_kernel<256>" and expected_proj_block(8193, 256, 768, (0, 0), (8, 24), 768) == "proj_wstat_kernel"
    # og_forward's 256-d batches, in launch order: the 2048-unit floor of proj_wstat_kernel and the 192 big tiles of the row-split GEMM
    wst, big2, t128 = "proj_wstat_kernel", "gemm_nt_f16x3_big2_kernel<2, 1>", "gemm_nt_f16x3_kernel<128, 2, RaggedNone, 2, 1>"
    ms, mf, ps, pst = k(256)
    assert forward_sequence(256, 12, 1024, 1024) == [wst, mf, big2, mf, t128, mf]        # 2304 units | 1536 units, 192 big tiles | 768 units, 96 big tiles
    assert forward_sequence(256, 16, 1024, 1024) == [wst, mf, wst, mf, t128, mf]         # the cross launch: 512 + 1536 = 2048 units; k | v: 1024 units, 128 big tiles
    gen = "gemm_nt_f16x3_kernel<128, 2, RaggedNone, 0, 0>"
    assert forward_sequence(256, 2, 128, 4100) == [gen, mf, gen, ps, ms, ps, mf]         # T = 8456, image 1 = 8200 rows: GEMMs of a partial last tile
    assert forward_sequence(256, 8, 0, 0, lens=RAGGED_LENS) == [big2, mf, big2, ps, ms, ps, mf]      # uniform, T0 = 512 and T1 = 22016 would give [wst, mf, wst, ms, ps, mf]
    assert forward_sequence(256, 1, 512, 22016) == [wst, mf, wst, ms, ps, mf]
    relu, plain = "gemm_nt_f16x3_kernel<128, 2, RaggedNone, 0, 0>", "gemm_nt_f16x3_kernel<128, 2, RaggedNone, 2, 1>"
    assert forward_sequence(128, 1, 128, 128, favor=True) == [relu, plain, "mlp_small_kernel<128>", relu, plain, relu, "mlp_small_kernel<128>", relu, plain,
                                                              "mlp_small_kernel<128>"]


# ----------------------------------------------------------------------------- shared plumbing of the GPU cases
gpu = pytest.mark.gpu
F16, I16 = torch.float16, torch.int16
SENT_BITS = torch.tensor(SENT, dtype=F16).view(I16).item()
EXTRA = 3                    # rows behind the matrix: NaN in the operands, the sentinel in the outputs


@pytest.fixture(scope="module", autouse=True)
def _threads():
    n = torch.get_num_threads()
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))      # float64 references beside the GPU
    yield
    torch.set_num_threads(n)
    for f in (_mlp_weights, _mlp_data, _proj_weights, _proj_data):   # the references and device operands of the last cases
        f.cache_clear()


def _bound(e32, ref):
    return max(2.0 * e32, 2e-6) + 2e-6 * ref.abs().max().item()


def _check(tag, got, ref, bound):
    """got against float64: finite, max |got - ref| < bound; prints the ratio."""
    assert got.shape == ref.shape, (tag, got.shape, ref.shape)
    assert torch.isfinite(got).all(), tag
    err = (got.double() - ref).abs().max().item()
    print(f"[proj/mlp forms] {tag}: err {err:.2e} bound {bound:.2e} ratio {err / bound:.3f}")
    assert err < bound, (tag, err, bound)


def _traced(fn):
    """-> the launches of mlp_fused.hip's four kernels fn made, in launch order."""
    return proj_mlp_instances(launched_kernels(fn))


def _as_given(t, scale=1.0):
    """fp32 [R, C] (C % 32 == 0) -> (hl32 rows of scale * t on the device, the values they hold / scale on the CPU)."""
    hl = ops.split_f16_hl((t * scale).to(_dev()).contiguous())
    return hl, ops.merge_f16_hl(hl).cpu() / scale


def _same_bits(a, b):
    return torch.equal(a.view(I16), b.view(I16))             # NaN != NaN: compare the halves as integers


# ----------------------------------------------------------------------------- 1. the message MLP
@functools.lru_cache(maxsize=2)
def _mlp_weights(D):
    """Asymmetric random weights at the scales of test_mlp_block_fused_vs_float64: the packed stream on the device, the values it holds
    (merge(split(256 w)) / 256), the biases (aligned, and at a 4-byte offset into a larger tensor)."""
    dev = _dev()
    g = torch.Generator().manual_seed(4000 + D)
    w0, w3 = torch.randn(2 * D, 2 * D, generator=g) * 0.04, torch.randn(D, 2 * D, generator=g) * 0.05
    b0, b3 = torch.randn(2 * D, generator=g) * 0.3, torch.randn(D, generator=g) * 0.3
    lib = _lib.load()
    st = torch.empty(lib.og_mlp_block_stream_bytes(D), dtype=torch.uint8)
    _lib.check(lib.og_mlp_block_pack(D, w0.data_ptr(), w3.data_ptr(), st.data_ptr()), "og_mlp_block_pack")
    off0, off3 = torch.zeros(2 * D + 4, device=dev), torch.zeros(D + 4, device=dev)
    off0[1:1 + 2 * D] = b0.to(dev); off3[1:1 + D] = b3.to(dev)
    d = dict(stream=st.to(dev), w0=_as_given(w0, 256.0)[1], w3=_as_given(w3, 256.0)[1], b0=b0, b3=b3, b0d=b0.to(dev), b3d=b3.to(dev),
             b0u=off0[1:1 + 2 * D], b3u=off3[1:1 + D], keep=(off0, off3))
    assert not (d["b0d"].data_ptr() | d["b3d"].data_ptr()) & 15 and d["b0u"].data_ptr() & 15 == 4 and d["b3u"].data_ptr() & 15 == 4
    return d


@functools.lru_cache(maxsize=2)
def _mlp_data(M, D):
    """[x | O] rows as the kernel is given them, float64 of x + W3 relu(W0 [x ; O] + b0) + b3 and e32 of the same in fp32 on the CPU."""
    w = _mlp_weights(D)
    g = torch.Generator().manual_seed(1000 + M)
    xo = torch.cat([torch.randn(M, D, generator=g) * 2.0, torch.randn(M, D, generator=g) * 1.5], 1)
    rows, xo_in = _as_given(xo)

    def run(dt):
        h = torch.relu(xo_in.to(dt) @ w["w0"].to(dt).T + w["b0"].to(dt))
        return xo_in[:, :D].to(dt) + h @ w["w3"].to(dt).T + w["b3"].to(dt)
    ref = run(torch.float64)
    return dict(rows=rows, ref=ref, e32=(run(torch.float32).double() - ref).abs().max().item())


def _mlp_buffer(d, M, D):
    """The rows in a buffer of ld = 4D + 8 halves with EXTRA rows behind them, NaN in every gap."""
    buf = torch.full((M + EXTRA, 4 * D + 8), NAN, dtype=F16, device=_dev())
    buf[:M, :4 * D] = d["rows"]
    return buf


def _run_mlp(M, D, b0="b0d", b3="b3d"):
    """One og_mlp_block launch -> (x [M, D] merged on the CPU, the launches).  Asserts that nothing but the x half of the rows changed."""
    w, d = _mlp_weights(D), _mlp_data(M, D)
    buf = _mlp_buffer(d, M, D)
    before = buf.clone()
    dev = _dev()
    inst = _traced(lambda: _lib.call("og_mlp_block", dev, D, buf.data_ptr(), 4 * D + 8, M, w["stream"].data_ptr(), w[b0].data_ptr(), w[b3].data_ptr(),
                                     _lib.STREAM))
    tag = f"mlp D={D} M={M}"
    assert _same_bits(buf[M:], before[M:]), f"{tag}: rows past M were written"
    assert _same_bits(buf[:M, 2 * D:], before[:M, 2 * D:]), f"{tag}: the O half or the gap of a row was written"
    return ops.merge_f16_hl(buf[:M, :2 * D].contiguous()).cpu(), inst


def _mlp_case(M, D, want, **kw):
    d = _mlp_data(M, D)
    got, inst = _run_mlp(M, D, **kw)
    assert inst == [want], (inst, want)
    _check(f"mlp D={D} M={M} {want} {kw or ''}", got, d["ref"], _bound(d["e32"], d["ref"]))
    return got


@gpu
@pytest.mark.parametrize("M", [1, 31, 32, 33, 8192])
@pytest.mark.parametrize("D", [256, 128])
def test_mlp_small(gpu_device, D, M):
    assert expected_mlp(M, D) == f"mlp_small_kernel<{D}>"
    _mlp_case(M, D, f"mlp_small_kernel<{D}>")


@gpu
@pytest.mark.parametrize("M", [8193, 8319, 8320])
@pytest.mark.parametrize("D", [256, 128])
def test_mlp_fused_by_size(gpu_device, D, M):
    """The smallest launches the 128-token kernel takes by size: 65 tiles, the last one holding 1 / 127 / 128 rows."""
    assert expected_mlp(M, D) == f"mlp_fused_kernel<{D}>"
    _mlp_case(M, D, f"mlp_fused_kernel<{D}>")


@gpu
@pytest.mark.parametrize("M", [1, 127, 128, 129, 200])
@pytest.mark.parametrize("D", [256, 128])
def test_mlp_unaligned_bias_takes_the_tile_kernel(gpu_device, D, M):
    """A bias that cannot be read as 16-byte vectors sends a launch of few rows to mlp_fused_kernel (og_launch_mlp_fused): one tile holding
    1 / 127 / 128 rows, two tiles.  The same operands with aligned biases run mlp_small_kernel; the two agree within the bound the existing
    test uses between the fused and the two-launch form."""
    d = _mlp_data(M, D)
    assert expected_mlp(M, D, b0_aligned=False) == expected_mlp(M, D, b3_aligned=False) == f"mlp_fused_kernel<{D}>"
    f0 = _mlp_case(M, D, f"mlp_fused_kernel<{D}>", b0="b0u")
    f3 = _mlp_case(M, D, f"mlp_fused_kernel<{D}>", b3="b3u")
    sm = _mlp_case(M, D, f"mlp_small_kernel<{D}>")
    tol = 2e-5 + 1e-6 * d["ref"].abs().max().item()
    assert torch.equal(f0, f3), "the same kernel on the same values"
    assert (f0 - sm).abs().max().item() < tol


@gpu
@pytest.mark.parametrize("what,code", [("ld_short", OG_E_ALIGN), ("ld_odd", OG_E_ALIGN), ("rows_off", OG_E_ALIGN), ("no_rows", OG_E_INVALID)])
@pytest.mark.parametrize("D", [256, 128])
def test_mlp_refusals(gpu_device, D, what, code):
    """og_launch_mlp_fused returns before any launch: the error code, and the buffer as it was."""
    M = 64
    w, d = _mlp_weights(D), _mlp_data(M, D)
    buf = _mlp_buffer(d, M, D)
    before = buf.clone()
    ld, rows, m = {"ld_short": (4 * D - 8, 0, M), "ld_odd": (4 * D + 4, 0, M), "rows_off": (4 * D + 8, 8, M), "no_rows": (4 * D + 8, 0, 0)}[what]
    rc = _lib.load().og_mlp_block(D, buf.data_ptr() + rows, ld, m, w["stream"].data_ptr(), w["b0d"].data_ptr(), w["b3d"].data_ptr(),
                                 torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == code, (what, rc)
    assert _same_bits(buf, before)


# ----------------------------------------------------------------------------- 2. the projections
@functools.lru_cache(maxsize=3)
def _proj_weights(N, K):
    dev = _dev()
    g = torch.Generator().manual_seed(5000 + N + K)
    w, bias = torch.randn(N, K, generator=g) * 0.06, torch.randn(N, generator=g) * 0.3
    lib = _lib.load()
    st = torch.empty(lib.og_proj_block_stream_bytes(N, K), dtype=torch.uint8)
    _lib.check(lib.og_proj_block_pack(N, K, w.data_ptr(), st.data_ptr()), "og_proj_block_pack")
    off = torch.zeros(N + 4, device=dev)
    off[1:1 + N] = bias.to(dev)
    return dict(stream=st.to(dev), w=_as_given(w, 256.0)[1], bias=bias, bias_d=bias.to(dev), bias_u=off[1:1 + N], keep=off,
                inv=torch.full((1,), 1.0 / 256.0, device=dev))


@functools.lru_cache(maxsize=2)
def _proj_data(M, N, K):
    """x as the kernel is given it, float64 x W^T + b over ALL N columns and e32 of the same in fp32 on the CPU."""
    w = _proj_weights(N, K)
    g = torch.Generator().manual_seed(2000 + M)
    x_hl, x_in = _as_given(torch.randn(M, K, generator=g) * 2.0)
    ref = x_in.double() @ w["w"].double().T + w["bias"].double()
    e32 = ((x_in @ w["w"].T + w["bias"]).double() - ref).abs().max().item()
    return dict(x_hl=x_hl, ref=ref, e32=e32)


def _proj_x(d, M, K):
    """X as og_forward passes it: [x | O] rows of 4K halves; NaN in the O half and in EXTRA rows behind the matrix."""
    X = torch.full((M + EXTRA, 4 * K), NAN, dtype=F16, device=_dev())
    X[:M, :2 * K] = d["x_hl"]
    return X


def _planes(M, ldy, off=0):
    """Two planes [M + EXTRA][ldy] in the sentinel, `off` halves into their allocation."""
    flat = [torch.full(((M + EXTRA) * ldy + off,), SENT, dtype=F16, device=_dev()) for _ in range(2)]
    return flat, [f[off:].view(M + EXTRA, ldy) for f in flat]


def _proj_case(M, K, N, a, b, want, split_row=0, ldy=None, plane_off=0):
    """One og_proj_block launch: the instance, every element inside a row's range against float64, every other element of both planes (the
    other columns, the ldy gap, the rows past M, what lies in front of a shifted plane) still the sentinel."""
    w, d = _proj_weights(N, K), _proj_data(M, N, K)
    dev = _dev()
    ldy = ldy if ldy is not None else N + (64 if want.startswith("proj_stream") else 4)
    X = _proj_x(d, M, K)
    flat, (yh, yl) = _planes(M, ldy, plane_off)
    if want.startswith("proj_stream"):
        assert not (yh.data_ptr() | yl.data_ptr()) & 127
    pred = expected_proj_block(M, K, N, a, b, ldy, split_row, planes_aligned=not (yh.data_ptr() | yl.data_ptr()) & 127)
    assert pred == want, (pred, want)
    inst = _traced(lambda: _lib.call("og_proj_block", dev, X.data_ptr(), 4 * K, M, K, N, w["stream"].data_ptr(), w["bias_d"].data_ptr(), w["inv"].data_ptr(),
                                     yh.data_ptr(), yl.data_ptr(), ldy, split_row, a[0], a[1], b[0], b[1], _lib.STREAM))
    assert inst == [want], (inst, want)
    tag = f"proj K={K} M={M} N={N} a={a} b={b} split={split_row} ldy={ldy} {want}"
    mask = torch.zeros(M + EXTRA, ldy, dtype=torch.bool)
    cut = 0 if split_row <= 0 else min(split_row, M)           # workgroups whose first row is below split_row take a: whole tiles, or every row
    mask[:cut, 32 * a[0]:32 * a[1]] = True
    mask[cut:M, 32 * b[0]:32 * b[1]] = True
    for name, f, p in (("hi", flat[0], yh), ("lo", flat[1], yl)):
        bits = p.cpu().view(I16)
        assert (bits[~mask] == SENT_BITS).all(), f"{tag}: the {name} plane was written outside the ranges"
        assert (f[:plane_off].cpu().view(I16) == SENT_BITS).all(), tag
    got = ops.merge_f16(yh, yl).cpu()[:M, :N]
    inside = mask[:M, :N]
    _check(tag, got[inside], d["ref"][inside], _bound(d["e32"], d["ref"]))


def _full(N):
    return (0, 0), (0, N // 32)


@gpu
@pytest.mark.parametrize("M", [1, 31, 32, 33])
@pytest.mark.parametrize("K", [256, 128])
def test_proj_small_full(gpu_device, K, M):
    _proj_case(M, K, 3 * K, *_full(3 * K), f"proj_small_kernel<{K}>")


@gpu
@pytest.mark.parametrize("K,M,parts", [(256, 2720, 3), (256, 2721, 1), (128, 4096, 2), (128, 4097, 1)])
def test_proj_small_deal_out_threshold(gpu_device, K, M, parts):
    """Both sides of tiles * parts <= 256 (launch_proj_small) on the whole q | k | v matrix: 85 x 3 / 86 x 3 at 24 blocks, 128 x 2 / 129 x 2 at
    12.  Not dealt out, a wave owns 3 blocks (K = 256) or 2 / 1 (K = 128)."""
    N = 3 * K
    assert proj_small_grid(M, *_full(N))[0] == parts
    _proj_case(M, K, N, *_full(N), f"proj_small_kernel<{K}>")


def _range_cases():
    out = []
    for K in (256, 128):
        for hi in (False, True):
            for nblk in (1, 3, 7, 8, 9, 12, 16, 20, 23, 24):
                M = 96 if not hi else 4128 if nblk <= 16 else 2752          # 129 x 2 and 86 x 3 workgroups: over the rule for that width
                for start in (0, 5):
                    b = (start, start + nblk)
                    parts, bpp, nb = proj_small_forms(M, (0, 0), b)
                    out.append(pytest.param(K, M, b, id=f"K{K}-M{M}-blocks{b[0]}to{b[1]}-parts{parts}-bpp{bpp}-perwave{'_'.join(map(str, nb))}"))
    return out


@gpu
@pytest.mark.parametrize("K,M,b", _range_cases())
def test_proj_small_ranges(gpu_device, K, M, b):
    """Column ranges of 1 .. 24 blocks of a 32-block matrix, from block 0 and from block 5, dealt out (M = 96) and not (M above the rule):
    every proj_small_run<NB>, waves of one workgroup with different NB (20 blocks: 3 / 2; 12: 2 / 1; 9 dealt out: a second part of one
    block), idle waves (1 .. 7 blocks)."""
    parts, bpp, nb = proj_small_forms(M, (0, 0), b)
    nblk = b[1] - b[0]
    assert (parts > 1) == (M == 96 and nblk > 8), (parts, bpp)
    _proj_case(M, K, 1024, (0, 0), b, f"proj_small_kernel<{K}>")


@gpu
@pytest.mark.parametrize("M,split,a_blocks", [(96, 32, None), (96, 64, None), (4128, 32, None), (4128, 64, None), (96, 32, 0), (96, 100, None)])
@pytest.mark.parametrize("K", [256, 128])
def test_proj_small_row_split(gpu_device, K, M, split, a_blocks):
    """The cross layer's launch: rows below split_row stop after the q blocks.  Dealt out (M = 96) and not (M = 4128); with an EMPTY range for
    the rows below the split (nothing of theirs may be written); split_row >= M (not a multiple of 32: every row takes the first range)."""
    a = (0, K // 32 if a_blocks is None else a_blocks)
    _proj_case(M, K, 3 * K, a, (0, 3 * K // 32), f"proj_small_kernel<{K}>", split_row=split)


@gpu
@pytest.mark.parametrize("N", [1024, 1152])
@pytest.mark.parametrize("K", [256, 128])
def test_proj_small_forced_deal_out(gpu_device, K, N):
    """More than 24 blocks are always dealt out: 32 blocks = 4 parts, 36 = 5 with a last part of 4 blocks (waves 4-7 idle)."""
    assert proj_small_grid(100, *_full(N))[:2] == (_cdiv(N // 32, 8), 8)
    _proj_case(100, K, N, *_full(N), f"proj_small_kernel<{K}>")


@gpu
@pytest.mark.parametrize("M", [8193, 8319, 8320])
@pytest.mark.parametrize("K", [256, 128])
def test_proj_stream_full(gpu_device, K, M):
    """The smallest launches the stage entry gives the 128-token kernel: 65 tiles, the last one holding 1 / 127 / 128 rows."""
    _proj_case(M, K, 3 * K, *_full(3 * K), f"proj_stream_kernel<{K}>")


@gpu
@pytest.mark.parametrize("K,pos", [(K, p) for K in (256, 128) for p in [*range(3 * K // 128), "kv"]])
def test_proj_stream_groups(gpu_device, K, pos):
    """One 128-channel group at every position of the matrix (six at K = 256, three at K = 128), and [K, 3K): the k | v of the updated image 0."""
    b = (K // 32, 3 * K // 32) if pos == "kv" else (4 * pos, 4 * pos + 4)
    _proj_case(8193, K, 3 * K, (0, 0), b, f"proj_stream_kernel<{K}>")


@gpu
@pytest.mark.parametrize("split", [128, 8192])
@pytest.mark.parametrize("K", [256, 128])
def test_proj_stream_row_split(gpu_device, K, split):
    _proj_case(8320, K, 3 * K, (0, K // 32), (0, 3 * K // 32), f"proj_stream_kernel<{K}>", split_row=split)


@gpu
@pytest.mark.parametrize("K", [256, 128])
def test_proj_stream_widest(gpu_device, K):
    """N = 1024: 8 groups, the most proj_stream_kernel takes (og_proj_step_check) (its bias area holds 1024 columns)."""
    _proj_case(8193, K, 1024, *_full(1024), f"proj_stream_kernel<{K}>")


@gpu
@pytest.mark.parametrize("why", ["n1152", "ldy", "ragged_range", "split_8224", "plane_off"])
@pytest.mark.parametrize("K", [256, 128])
def test_proj_fall_backs(gpu_device, K, why):
    """Above 8192 rows the stage entry still gives proj_small_kernel what the stream kernel cannot take: a range wider than 8 groups, plane rows
    that are not whole 64-half lines, a range that is not whole groups, a split row that is a multiple of 32 but not of 128, a plane that
    is not 128-byte aligned."""
    N, want = 3 * K, f"proj_small_kernel<{K}>"
    if why == "n1152":
        _proj_case(8193, K, 1152, *_full(1152), want, ldy=1152 + 64)
    elif why == "ldy":
        _proj_case(8193, K, N, *_full(N), want, ldy=N + 4)
    elif why == "ragged_range":
        _proj_case(8193, K, N, (0, 0), (0, N // 32 - 2), want, ldy=N + 64)
    elif why == "split_8224":
        _proj_case(8320, K, N, (0, K // 32), (0, N // 32), want, split_row=8224, ldy=N + 64)
    else:
        _proj_case(8193, K, N, *_full(N), want, ldy=N + 64, plane_off=32)


@gpu
@pytest.mark.parametrize("what,code", [("split_33", OG_E_SHAPE), ("bias_off", OG_E_ALIGN), ("ld_short", OG_E_SHAPE), ("range_past_n", OG_E_SHAPE)])
@pytest.mark.parametrize("K", [256, 128])
def test_proj_refusals(gpu_device, K, what, code):
    """og_proj_block / og_launch_proj return before any launch: the error code, and both planes as they were."""
    M, N = 96, 3 * K
    w, d = _proj_weights(N, K), _proj_data(M, N, K)
    X = _proj_x(d, M, K)
    flat, (yh, yl) = _planes(M, N + 4)
    nb = N // 32
    split, bias, ld, a1 = {"split_33": (33, "bias_d", 4 * K, nb), "bias_off": (0, "bias_u", 4 * K, nb), "ld_short": (0, "bias_d", 2 * K - 8, nb),
                           "range_past_n": (0, "bias_d", 4 * K, nb + 1)}[what]
    rc = _lib.load().og_proj_block(X.data_ptr(), ld, M, K, N, w["stream"].data_ptr(), w[bias].data_ptr(), w["inv"].data_ptr(), yh.data_ptr(), yl.data_ptr(),
                                  N + 4, split, 0, K // 32, 0, a1, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == code, (what, rc)
    for f in flat:
        assert (f.cpu().view(I16) == SENT_BITS).all()


# ----------------------------------------------------------------------------- 3. the forms og_forward launches
def _model(D, tweak=None, heads=4, attention="softmax", iters=2):
    from tests.test_gpu_parity import _build
    cfg = syn.make_config(descriptor_dim=D, num_stages=1, num_heads=heads, num_iters=iters, side_info_size=1, residual=True, attention=attention)
    sd = syn.make_state_dict(cfg, seed=0)
    if tweak is not None:
        tweak(sd, D)
    return cfg, sd, _build(cfg, sd, _dev())


def _distinct_prescales(sd, D):
    """Single entries of both layers' k, fc.0 and fc.3 weights so large that put_matrix (api.hip:324, 353, 368) must give the three matrices
    of a layer the pre-scales 128, 64 and 32 instead of 256 -- placed where they multiply an exact zero, so the layer computes what it
    would without them: the q channel that meets the large k channel is zeroed, the hidden channel the large fc.0 entry feeds is dead
    (bias -1e4 under the ReLU), and the large fc.3 entry multiplies that dead channel, whose BatchNorm shift is zeroed."""
    for l in (0, 1):
        p = f"attention_gnn.layers.{l}.module"
        c, o = 5 + l, 9 + 2 * l
        sd[f"{p}.mha.in_proj_q.weight"][c] = 0.0
        sd[f"{p}.mha.in_proj_q.bias"][c] = 0.0
        sd[f"{p}.mha.in_proj_k.weight"][c, 3, 0] = 150.0           # 256 x 150 > 32768 >= 128 x 150
        sd[f"{p}.fc.0.weight"][o, 7, 0] = 300.0                    # 128 x 300 > 32768 >= 64 x 300
        sd[f"{p}.fc.0.bias"][o] = -1e4
        sd[f"{p}.fc.2.bias"][o] = 0.0
        sd[f"{p}.fc.2.running_mean"][o] = 0.0
        gain = (sd[f"{p}.fc.2.weight"][o] / torch.sqrt(sd[f"{p}.fc.2.running_var"][o] + 1e-5)).item()
        sd[f"{p}.fc.3.weight"][11, o, 0] = 700.0 / gain            # 64 x 700 > 32768 >= 32 x 700 after the BatchNorm fold


def _layer64(sd, H, l, x0, x1, attention="softmax"):
    """attention_gnn.layers[l] in float64 on [B, m, D], [B, n, D] (attention_gnn.py:63-77), one pair at a time (a 4100 x 4100 attention matrix
    per head is 134 MB)."""
    p = f"attention_gnn.layers.{l}.module"
    mp = lambda q, kv: torch.cat([orc.message_passing(q[i:i + 1], kv[i:i + 1], sd, p, H, False, attention=attention) for i in range(q.shape[0])])
    with torch.no_grad():
        if l % 2 == 0:
            return mp(x0, x0), mp(x1, x1)
        r0 = mp(x0, x1)
        return r0, mp(x1, r0)                                      # image 1 against the UPDATED image 0


FORWARD_CASES = [pytest.param(128, 2, 128, 4100, None, id="d128-B2-m128-n4100"), pytest.param(128, 2, 130, 4100, None, id="d128-B2-m130-n4100"),
                 pytest.param(256, 1, 128, 160, None, id="d256-B1-m128-n160"), pytest.param(256, 1, 130, 97, None, id="d256-B1-m130-n97"),
                 pytest.param(256, 2, 128, 4100, None, id="d256-B2-m128-n4100"), pytest.param(128, 2, 128, 4100, "prescales", id="d128-B2-m128-n4100-prescales"),
                 pytest.param(256, 12, 1024, 1024, None, id="d256-B12-m1024-n1024"), pytest.param(256, 16, 1024, 1024, None, id="d256-B16-m1024-n1024"),
                 pytest.param(128, 1, 128, 128, "favor", id="d128-B1-m128-n128-favor_relu")]
ENC_TAIL, TAIL = 2, 3        # split-f16 GEMM launches of a forward in front of the GNN (the last encoder conv, per image: hidden width 128 <= D) and behind it
                             # (the final projection per image, the score matrix)
RAGGED_LENS = ([40, 88, 64, 64, 100, 28, 64, 64], [2752, 2700, 2804, 2752, 2600, 2904, 2752, 2752])      # T0 = 512, T1 = 22016


def _gnn_launches(fn, D):
    """-> every projection and message-MLP launch of the GNN of one traced forward, in launch order (the GEMMs around the GNN checked and cut off)."""
    seq = projection_candidates(launched_kernels(fn))
    assert len(seq) > ENC_TAIL + TAIL and all(k.startswith("gemm_nt_f16x3_") for k in seq[:ENC_TAIL] + seq[-TAIL:]), seq
    return seq[ENC_TAIL:-TAIL]


@gpu
@pytest.mark.parametrize("D,B,m,n,variant", FORWARD_CASES)
def test_forward_forms(gpu_device, D, B, m, n, variant):
    """One stage of og_forward: EVERY projection and message-MLP launch, in launch order, against the restatement (tests/proj_plan_ref.py), then x after
    the self layer and after the cross layer against float64 of that layer applied to the x the call itself showed one tap earlier.
      d128 m128 n4100 (T0 = 256, T = 8456): the stream launch of the self layer, the stream launch with a row split, proj_small for the k | v of
                         the updated image 0, mlp_fused<128> for the self layer and side 1, mlp_small<128> for side 0
      d128 m130 n4100 (T0 = 260): no row split -- a stream launch at row offset T0 and proj_small for image 0's q
      d256 m128 n160 / m130 n97: one proj_small launch with a row split / three proj_small launches in the cross layer
      d256 m128 n4100: mlp_fused<256> under the forward (scales_dev set); the self launch and image 1's q | k | v (8200 rows) are 128-tile GEMMs
      d256 B12 m1024 n1024 (T0 = 12288): 2304 units -> proj_wstat_kernel for the self layer; the cross launch has 1536 units (below the 2048-unit
                         floor) and exactly 192 big tiles -> the row-split big2 GEMM; the k | v has 768 units and 96 big tiles -> the 128-token tile GEMM
      d256 B16 m1024 n1024 (T0 = 16384): the cross launch counts T0 / 32 + ceil(T1 / 32) * 3 = 512 + 1536 = 2048 units -> ONE proj_wstat launch with the row split
      d128 favor_relu (one head, QW = 5 D): no fragment-major copy exists, every projection is a tile GEMM; a range that spans the feature and value
                         blocks is TWO launches (ReLU / none), image 0's q in the cross layer one
      prescales: the multipliers {1 / S_qkv, 1 / S_0, 1 / S_3} of both layers are pairwise different (asserted from the packed blob)"""
    from tests.packed_model import layout_of
    prescales, favor = variant == "prescales", variant == "favor"
    H, att = (1, "favor_relu") if favor else (4, "softmax")
    cfg, sd, model = _model(D, _distinct_prescales if prescales else None, heads=H, attention=att, iters=2 if B < 12 and not favor else 3)
    if prescales:
        L, blob = layout_of(model), model.pack_host()
        for l in (0, 1):
            o = L.layer0 + l * L.layer_stride + L.o_scale
            sq, s0, s3 = (float(v) for v in blob[o:o + 3])
            assert (sq, s0, s3) == (1.0 / 128, 1.0 / 64, 1.0 / 32), (l, sq, s0, s3)
            assert len({sq, s0, s3, 1.0 / 256}) == 4
    data = syn.make_batch(B, m, n, D, 1, seed=41 + m)
    dd = to_device(data, _dev())
    taps = [tuple(t.cpu() for t in model.forward_tap(dd, k)) for k in (0, 1)]
    box = []
    inst = _gnn_launches(lambda: box.append(model.forward_tap(dd, 2)), D)
    taps.append(tuple(t.cpu() for t in box[0]))
    want = forward_sequence(D, B, m, n, favor=favor)
    assert inst == want, (inst, want)
    tag = f"forward D={D} B={B} m={m} n={n}{' ' + variant if variant else ''}"
    for l in (0, 1):
        r0, r1 = _layer64(sd, H, l, taps[l][0].double(), taps[l][1].double(), att)
        scale = max(1.0, r0.abs().max().item(), r1.abs().max().item())
        _check(f"{tag} layer {l} image 0", taps[l + 1][0], r0, TOL_TAP * scale)
        _check(f"{tag} layer {l} image 1", taps[l + 1][1], r1, TOL_TAP * scale)


@gpu
def test_forward_forms_ragged_batch(gpu_device):
    """og_forward_ragged at 256-d, 8 pairs, T0 = 512 and T1 = 22016 token rows: as a uniform batch these counts would put the self launch (2112 units)
    and the cross launch (2080 units, 260 big tiles, T0 and T whole tiles) on proj_wstat_kernel with a row split (asserted from the restatement); a
    ragged batch takes neither the weight-stationary kernel nor a row-split launch -- big2 GEMMs, and image 0's q as a launch of its own.
    og_forward_tap has no ragged form: every pair's scores against the same pair's own call (tests/test_gpu_parity.py: test_ragged_packed_wide_range)."""
    D = 256
    cfg, sd, model = _model(D, iters=3)
    cpu = []
    for i, (m, n) in enumerate(zip(*RAGGED_LENS)):
        p = syn.make_pair(m, n, D, 1, seed=900 + i)
        p["image0_size"] = list(syn.IMAGE_WH); p["image1_size"] = list(syn.IMAGE_WH)
        cpu.append(p)
    pairs = [to_device(p, _dev()) for p in cpu]
    box = []
    inst = _gnn_launches(lambda: box.append(model.match_ragged(pairs, 0.2)), D)
    want = forward_sequence(D, len(cpu), 0, 0, lens=RAGGED_LENS)
    assert inst == want, (inst, want)
    assert "proj_wstat_kernel" not in inst and inst.count("gemm_nt_f16x3_big2_kernel<2, 1>") == 2
    assert forward_sequence(D, 1, sum(RAGGED_LENS[0]), sum(RAGGED_LENS[1])).count("proj_wstat_kernel") == 2
    for p, r, m, n in zip(pairs, box[0], *RAGGED_LENS):
        one = {k: (v[None] if torch.is_tensor(v) else v) for k, v in p.items()}
        ref = model.match(one, 0.2)
        assert r["scores"].shape == (m + 1, n + 1)
        err = (r["scores"] - ref["scores"][0]).abs().max().item()
        print(f"[proj/mlp forms] ragged pair {m}x{n}: scores against its own call, err {err:.2e}")
        assert err < 1e-4, (m, n, err)
