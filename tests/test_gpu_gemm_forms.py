"""Every exact-fp32 and split-f16 GEMM form the default dispatch launches, pinned to float64 on EVERY output element, with the launched
instance asserted.

og_launch_gemm (csrc/gemm_f32.hip) and og_launch_gemm_f16x3 (csrc/gemm_f16x3.hip) pick one of about two dozen template instances from the
shape and the epilogue.  `expected_f32` / `expected_f16x3` below restate those rules; every GPU case asserts that the GEMM instances it
launched are exactly the predicted ones (sections 1, 2) or contain it (section 3, whole forward calls), so a change of the dispatch has to
be a deliberate change of this file, and a case cannot drift onto another kernel unnoticed.

  0. the restatement itself, on both sides of every boundary (CPU)
  1. exact fp32 through _lib (og_gemm_nt, og_gemm_kmajor, og_scores, og_splitk_reduce): both tile heights for each operand layout, K of 4 /
     36 / 68 / 96, tile edges, every epilogue on both tiles, NaN in every operand gap and a sentinel around the output, split-K with a ragged
     and with an EMPTY last chunk, the reduction at the ends of its 16-wide and 4-wide loops
  2. split-f16 through og_gemm_nt_f16x3 / og_gemm_nt_f16x3_reshl: the seven epilogue instances of the 256-tile kernel on three grids (48 x 4,
     192 x 1, 50 x 4 = padded block ids), the 128-tile specialisations and the generic instance, the 64-wide kernel, res_hl aliasing the
     output, NaN halves in the operand gaps and a sentinel around the output
  3. the forms only og_forward / og_forward_ragged launch, through SuperGlue: the final projection (alpha + Ct, ct_rag 1 / 2) from the
     residual stream at the last tap, the score launch (one pair, small batch, big_kernel<RaggedNone>, big_kernel<RaggedDesc>) from the
     returned context descriptors, the row-split q | k | v launch of a cross layer

Tolerance: e32 = the max error of the CPU fp32 product of the same operands against float64, measured in the case; the bound is
max(2 e32, 1e-6), + 2e-6 max|ref| where the output is a (hi, lo) pair, on the whole output.  relu == 2: 30 x that bound (d/dv sin(30 v)).
Split-f16 operands: the reference is float64 on merge(split(x)), what the kernel is given.  Every case prints err / bound.

instance -> a case that asserts it
  gemm_nt_f32_kernel<64, 64, false, false, RaggedNone>      test_f32_both_tiles[nt-8064...], test_f32_edges, test_f32_epilogues[short-...]
  gemm_nt_f32_kernel<128, 64, false, false, RaggedNone>     test_f32_both_tiles[nt-8065...], test_f32_epilogues[tall-...], test_f32_batched
  gemm_nt_f32_kernel<64 | 128, 64, false, true, RaggedNone> test_f32_both_tiles[nk-...]
  gemm_nt_f32_kernel<64 | 128, 64, true, true, RaggedNone>  test_f32_both_tiles[kk-...], test_f32_doubly_kmajor_scalar_tail, test_f32_split_k
  gemm_nt_f16x3_big2_kernel<1, 2 | 1, 3 | 1, 1 | 1, 0 | 2, 1 | 2, 0 | 0, 0>   test_f16x3_big2_epilogues (each on three grids)
  gemm_nt_f16x3_big_kernel<RaggedNone>                      test_forward_scores_big_batch
  gemm_nt_f16x3_big_kernel<RaggedDesc>                      test_forward_scores_big_batch_ragged
  gemm_nt_f16x3_kernel<128, 2, RaggedNone, 1, 2 | 1, 1 | 1, 3 | 2, 1>   test_f16x3_tile128_whole, test_f16x3_191_tiles_fall_back
  gemm_nt_f16x3_kernel<128, 2, RaggedNone, 0, 0>            test_f16x3_tile128_generic, test_f16x3_bare_fp32_odd_n, test_forward_final_projection
  gemm_nt_f16x3_kernel<128, 2, RaggedDesc, 0, 0>            test_forward_final_projection_ragged
  gemm_nt_f16x3_kernel<64, 2, RaggedNone, 0, 0>             test_f16x3_tile64
  gemm_nt_f16x3_kernel<64, 2, RaggedDesc, 0, 0>             test_forward_ragged_narrow_scores
not covered, and why:
  gemm_nt_f32_kernel<128, 128, ...>       needs OG_GEMM_F32_BN=128: an experiment, never the default
  gemm_nt_f32_kernel<..., RaggedDesc>     compiled, but no caller passes a ragged descriptor to the fp32 launcher (og_forward_ragged forms its
                                          scores on the split-f16 kernel), and the public entries cannot
  gemm_nt_f16x3_big_kernel at nz == 1     the first generation: only with OG_GEMM_BIG2=0 or OG_GEMM_TILE=256
"""
import functools
import os

import pytest
import torch

from openglue_amd import _lib, ops, synthetic as syn
from openglue_amd.kernel_trace import gemm_instances, launched_kernels
from oracle import superglue_oracle as orc
from tests.util import to_device

# The dispatch knobs are read once per process: one left in the environment would move every case below to another kernel.
_KNOBS = sorted(k for k in os.environ if k.startswith("OG_GEMM_"))
if _KNOBS:
    raise RuntimeError(f"test_gpu_gemm_forms runs the default dispatch: unset {_KNOBS}")


def _cdiv(a, b):
    return (a + b - 1) // b


# ----------------------------------------------------------------------------- 0. the selection rules, restated
def expected_f32(M, N, K, batch=1, a_kmajor=False, b_kmajor=False):
    """The instance og_launch_gemm (gemm_f32.hip) launches in the default environment.  The 128 x 128 tile needs
    OG_GEMM_F32_BN=128 (experiment-only): out of scope here.  No caller passes a ragged descriptor: RaggedNone always."""
    bm = 128 if _cdiv(M, 128) * batch * _cdiv(N, 64) >= 1024 else 64          # narrow / shortt there
    tf = lambda b: "true" if b else "false"
    return f"gemm_nt_f32_kernel<{bm}, 64, {tf(a_kmajor)}, {tf(b_kmajor)}, RaggedNone>"


EM_RUNTIME, EM_NONE, EM_RELU, EM_RES_HL = 0, 1, 2, 3          # gemm_f16x3.hip:298


def expected_f16x3(M, N, K, batch=1, c32=False, planes=False, hl=False, relu=False, res32=False, res_hl=False, alpha=False, ct=False,
                   ragged=False):
    """The instance og_launch_gemm_f16x3 (gemm_f16x3.hip) launches in the default environment.  planes / hl: the split-f16
    output as two planes (Ch, Cl) or as hl32 rows; M, N of a ragged launch: the largest pair's."""
    nz = batch if batch > 1 else 1
    rd = "RaggedDesc" if ragged else "RaggedNone"
    ch = planes or hl
    fits = (N % 256 == 0 or nz > 1) and _cdiv(M, 256) * _cdiv(N, 256) * nz >= 192 and not alpha and not ct          # gemm_big_tile_allowed
    if fits:
        if nz == 1 and not ragged:                                                                                   # gemm_big2_allowed
            whole = M % 256 == 0 and N % 256 == 0 and ch and not c32
            em = EM_RUNTIME
            if not res32 and not res_hl:
                em = EM_RELU if relu else EM_NONE
            elif not relu and res_hl:
                em = EM_RES_HL
            if whole and hl:
                return f"gemm_nt_f16x3_big2_kernel<1, {em}>"
            if whole and planes:
                return f"gemm_nt_f16x3_big2_kernel<2, {em if em == EM_NONE else EM_RUNTIME}>"
            return "gemm_nt_f16x3_big2_kernel<0, 0>"
        return f"gemm_nt_f16x3_big_kernel<{rd}>"
    if N > 64:
        if not ragged:
            whole = nz == 1 and M % 128 == 0 and N % 128 == 0 and ch and not c32 and not ct and not alpha and not res32
            if whole:
                if hl and not res_hl and relu: return "gemm_nt_f16x3_kernel<128, 2, RaggedNone, 1, 2>"
                if hl and not res_hl and not relu: return "gemm_nt_f16x3_kernel<128, 2, RaggedNone, 1, 1>"
                if hl and res_hl and not relu: return "gemm_nt_f16x3_kernel<128, 2, RaggedNone, 1, 3>"
                if planes and not res_hl and not relu: return "gemm_nt_f16x3_kernel<128, 2, RaggedNone, 2, 1>"
        return f"gemm_nt_f16x3_kernel<128, 2, {rd}, 0, 0>"
    return f"gemm_nt_f16x3_kernel<64, 2, {rd}, 0, 0>"


def test_restatement_sides_of_the_boundaries():
    """The boundaries of both launchers as the restatement sees them (a wrong restatement would make every assertion below pointless)."""
    short, tall = "gemm_nt_f32_kernel<64, 64, false, false, RaggedNone>", "gemm_nt_f32_kernel<128, 64, false, false, RaggedNone>"
    assert expected_f32(4224, 1984, 36) == short                     # 33 x 31 = 1023 workgroups of 128 x 64
    assert expected_f32(4096, 2048, 36) == tall                      # 32 x 32 = 1024
    assert expected_f32(8064, 1024, 36) == short and expected_f32(8065, 1024, 36) == tall          # 63 x 16, 64 x 16
    assert expected_f32(1100, 520, 36, batch=15) == tall and expected_f32(1000, 440, 36, batch=16) == short   # 9 x 15 x 9, 8 x 16 x 7
    assert expected_f32(8065, 1022, 37, 1, True, True) == "gemm_nt_f32_kernel<128, 64, true, true, RaggedNone>"
    assert expected_f32(300, 200, 36, 1, False, True) == "gemm_nt_f32_kernel<64, 64, false, true, RaggedNone>"
    # 191 and 192 256-tiles
    assert expected_f16x3(191 * 256, 256, 32, hl=True, relu=True) == "gemm_nt_f16x3_kernel<128, 2, RaggedNone, 1, 2>"
    assert expected_f16x3(192 * 256, 256, 32, hl=True, relu=True) == "gemm_nt_f16x3_big2_kernel<1, 2>"
    assert expected_f16x3(12288, 1024, 96, planes=True) == "gemm_nt_f16x3_big2_kernel<2, 1>"
    assert expected_f16x3(12288 - 256, 1024, 96, planes=True) == "gemm_nt_f16x3_kernel<128, 2, RaggedNone, 2, 1>"
    # whole and non-whole M (256-tile and 128-tile), an fp32 output beside the rows
    assert expected_f16x3(12288, 1024, 96, hl=True, res_hl=True) == "gemm_nt_f16x3_big2_kernel<1, 3>"
    assert expected_f16x3(12288 - 5, 1024, 96, hl=True, res_hl=True) == "gemm_nt_f16x3_big2_kernel<0, 0>"
    assert expected_f16x3(12288, 1024, 96, hl=True, c32=True) == "gemm_nt_f16x3_big2_kernel<0, 0>"
    assert expected_f16x3(12288, 1024, 96, hl=True, relu=True, res_hl=True) == "gemm_nt_f16x3_big2_kernel<1, 0>"
    assert expected_f16x3(12288, 1024, 96, hl=True, res32=True) == "gemm_nt_f16x3_big2_kernel<1, 0>"
    assert expected_f16x3(12288, 1024, 96, planes=True, relu=True) == "gemm_nt_f16x3_big2_kernel<2, 0>"
    assert expected_f16x3(12288, 1024 + 32, 96, hl=True) == "gemm_nt_f16x3_kernel<128, 2, RaggedNone, 0, 0>"       # N % 256 != 0 at nz == 1
    assert expected_f16x3(256, 256, 96, hl=True) == "gemm_nt_f16x3_kernel<128, 2, RaggedNone, 1, 1>"
    assert expected_f16x3(255, 256, 96, hl=True) == "gemm_nt_f16x3_kernel<128, 2, RaggedNone, 0, 0>"
    assert expected_f16x3(256, 256, 96, hl=True, relu=True, res_hl=True) == "gemm_nt_f16x3_kernel<128, 2, RaggedNone, 0, 0>"
    # N = 64 and 65
    assert expected_f16x3(128, 64, 96, hl=True) == "gemm_nt_f16x3_kernel<64, 2, RaggedNone, 0, 0>"
    assert expected_f16x3(130, 65, 96, c32=True) == "gemm_nt_f16x3_kernel<128, 2, RaggedNone, 0, 0>"
    # the forward's own launches: final projection (alpha, Ct), scores of one pair / a small batch / 3 x 2048 x 2048, ragged twins
    assert expected_f16x3(3 * 130, 256, 256, hl=True, res32=True, alpha=True, ct=True) == "gemm_nt_f16x3_kernel<128, 2, RaggedNone, 0, 0>"
    assert expected_f16x3(49152, 256, 256, hl=True, ct=True) == "gemm_nt_f16x3_kernel<128, 2, RaggedNone, 0, 0>"
    assert expected_f16x3(130, 97, 256, batch=3, c32=True) == "gemm_nt_f16x3_kernel<128, 2, RaggedNone, 0, 0>"
    assert expected_f16x3(2048, 2048, 256, batch=3, c32=True) == "gemm_nt_f16x3_big_kernel<RaggedNone>"
    assert expected_f16x3(2048, 2048, 256, batch=2, c32=True) == "gemm_nt_f16x3_kernel<128, 2, RaggedNone, 0, 0>"   # 128 tiles
    assert expected_f16x3(2048, 2048, 256, batch=3, c32=True, ragged=True) == "gemm_nt_f16x3_big_kernel<RaggedDesc>"
    assert expected_f16x3(130, 60, 256, batch=2, c32=True, ragged=True) == "gemm_nt_f16x3_kernel<64, 2, RaggedDesc, 0, 0>"


# ----------------------------------------------------------------------------- shared plumbing of the GPU cases
gpu = pytest.mark.gpu
NAN = float("nan")
SENT = -777.25               # exactly representable in fp32 and binary16


@pytest.fixture(scope="module", autouse=True)
def _threads():
    n = torch.get_num_threads()
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))      # float64 references beside the GPU
    yield
    torch.set_num_threads(n)
    for f in (_f32_data, _h_data):       # the references and device operands of the last cases
        f.cache_clear()


@pytest.fixture(autouse=True)
def _stop_after_a_gpu_fault(request):
    """A HIP error ends the run: nothing more is launched on a device that has faulted."""
    yield
    if "gpu_device" in request.fixturenames:
        try:
            torch.cuda.synchronize()
        except RuntimeError as e:
            pytest.exit(f"HIP error after {request.node.name}: {e}", returncode=3)


def _dev():
    return torch.device("cuda:0")


def _traced(fn):
    """-> (the set of GEMM instances fn launched, every kernel name in launch order)."""
    names = launched_kernels(fn)
    return gemm_instances(names), names


def _round4(x):
    return (x + 3) // 4 * 4


def _gapped(mat, ld, extra_rows, fill):
    """cpu [Z, R, C] -> device [Z, R + extra_rows, ld] holding `fill` everywhere but in the corner that holds mat."""
    Z, R, C = mat.shape
    buf = torch.full((Z, R + extra_rows, ld), fill, dtype=mat.dtype)
    buf[:, :R, :C] = mat
    return buf.to(_dev())


def _bound(e32, ref, hl=False, factor=1.0):
    return factor * (max(2.0 * e32, 1e-6) + (2e-6 * ref.abs().max().item() if hl else 0.0))


def _check(tag, got, ref, bound):
    """The whole output against float64: finite, max |got - ref| < bound; prints the ratio."""
    assert got.shape == ref.shape, (tag, got.shape, ref.shape)
    assert torch.isfinite(got).all(), tag
    err = (got.double() - ref).abs().max().item()
    print(f"[gemm forms] {tag}: err {err:.2e} bound {bound:.2e} ratio {err / bound:.3f}")
    assert err < bound, (tag, err, bound)


def _untouched(tag, buf, rows, cols, sent=SENT):
    """buf [..., R, ld]: everything outside [..., :rows, :cols] still holds the sentinel, bit for bit."""
    assert (buf[..., rows:, :] == sent).all(), f"{tag}: rows past M were written"
    assert (buf[..., :rows, cols:] == sent).all(), f"{tag}: the gap columns of the output were written"


# ----------------------------------------------------------------------------- 1. exact fp32
@functools.lru_cache(maxsize=2)
def _f32_data(Z, M, N, K, sa=3.0):
    """Logical operands A [Z, M, K] (randn x sa), B [Z, N, K] (randn x 0.05), float64 A B^T and e32 of the CPU fp32 product."""
    g = torch.Generator().manual_seed(Z * 1000003 + M * 7919 + N * 31 + K)
    A, B = torch.randn(Z, M, K, generator=g) * sa, torch.randn(Z, N, K, generator=g) * 0.05
    ref = A.double() @ B.double().transpose(1, 2)
    e32 = ((A @ B.transpose(1, 2)).double() - ref).abs().max().item()
    bias, res, alpha = torch.randn(N, generator=g) * 0.3, torch.randn(Z, M, N, generator=g) * 0.5, torch.rand(N, generator=g)
    return A, B, ref, e32, bias, res, alpha


def _run_f32(layout, A, B, pad, bias=None, relu=0, res=None, alpha=None, scale=1.0, inplace=False):
    """One launch of og_gemm_nt ("nt") or og_gemm_kmajor ("nk": B k-major, "kk": both) on operands stored with `pad` NaN floats after
    every row and three NaN rows after every matrix (so every batch stride has a gap too); the output lies in a sentinel.
    -> (C [Z, M, N] on the CPU, the GEMM instances launched)."""
    Z, M, K = A.shape
    N = B.shape[1]
    dev = _dev()
    er = 3 if pad else 0
    Ast = A.transpose(1, 2) if layout == "kk" else A
    Bst = B if layout == "nt" else B.transpose(1, 2)
    lda, ldb, ldc = _round4(Ast.shape[2]) + pad, _round4(Bst.shape[2]) + pad, _round4(N) + pad
    Ad, Bd = _gapped(Ast, lda, er, NAN), _gapped(Bst, ldb, er, NAN)
    Cd = torch.full((Z, M + er, ldc), SENT, device=dev)
    sA, sB, sC = Ad.shape[1] * lda, Bd.shape[1] * ldb, (M + er) * ldc
    rp, ldr = None, 0
    if inplace:                                  # C is res: the epilogue reads the residual from the element it then overwrites
        assert Z == 1
        Cd[:, :M, :N] = res.to(dev)
        rp, ldr = Cd.data_ptr(), ldc
    elif res is not None:                        # og_gemm_nt takes the residual's batch stride as M * ldr: no rows between its matrices
        Rd = _gapped(res, _round4(N) + pad, 0, NAN)
        rp, ldr = Rd.data_ptr(), _round4(N) + pad
    bd = bias.to(dev) if bias is not None else None
    ad = alpha.to(dev) if alpha is not None else None
    if layout == "nt":
        fn = lambda: _lib.call("og_gemm_nt", dev, Ad.data_ptr(), lda, sA, Bd.data_ptr(), ldb, sB, Cd.data_ptr(), ldc, sC, M, N, K, Z,
                               _lib.ptr(bd), relu, rp, ldr, _lib.ptr(ad), float(scale), _lib.STREAM)
    else:
        assert bias is None and res is None and not relu         # og_gemm_kmajor has the scale only
        fn = lambda: _lib.call("og_gemm_kmajor", dev, Ad.data_ptr(), lda, sA, int(layout == "kk"), Bd.data_ptr(), ldb, sB, Cd.data_ptr(), ldc, sC,
                               M, N, K, Z, 0, 0, float(scale), _lib.STREAM)
    inst, _ = _traced(fn)
    out = Cd.cpu()
    _untouched(f"{layout} {Z}x{M}x{N}x{K}", out, M, N)
    return out[:, :M, :N], inst


def _epilogue64(ref, bias=None, relu=0, res=None, alpha=None, scale=1.0):
    """gemm_f32.hip:209-216 in float64."""
    v = ref if bias is None else ref + bias.double()
    if relu == 1:
        v = torch.relu(v)
    elif relu == 2:
        v = torch.sin(30.0 * v)
    if res is not None:
        v = alpha.double() * v + (1.0 - alpha.double()) * res.double() if alpha is not None else v + res.double()
    return v * scale


LAYOUTS = {"nt": (False, False), "nk": (False, True), "kk": (True, True)}


def _f32_case(layout, Z, M, N, K, pad, want_bm=None, scale=1.0):
    A, B, ref, e32, *_ = _f32_data(Z, M, N, K)
    want = expected_f32(M, N, K, Z, *LAYOUTS[layout])
    if want_bm is not None:
        assert want.startswith(f"gemm_nt_f32_kernel<{want_bm}, 64,"), want
    got, inst = _run_f32(layout, A, B, pad, scale=scale)
    assert inst == {want}, (inst, want)
    _check(f"f32 {layout} Z={Z} {M}x{N}x{K} pad={pad} {want}", got, ref * scale, _bound(e32 * scale, ref))


# M = 8064 / 8065 at N = 1024: 63 x 16 = 1008 and 64 x 16 = 1024 workgroups of 128 x 64 -> the 64-row and the 128-row tile, the latter with
# a last M-tile of ONE row.  K = 4: a partial k-tile; 36 / 68 / 96: one, two and three passes of the prefetch loop, the last one partial.
@gpu
@pytest.mark.parametrize("layout", ["nt", "nk", "kk"])
@pytest.mark.parametrize("M,bm", [(8064, 64), (8065, 128)])
@pytest.mark.parametrize("K", [4, 36, 68, 96])
def test_f32_both_tiles(gpu_device, layout, K, M, bm):
    _f32_case(layout, 1, M, 1024, K, pad=4, want_bm=bm)


@gpu
@pytest.mark.parametrize("M,N,K,bm", [(8062, 1022, 37, 64), (8065, 1022, 37, 128), (131, 67, 37, 64), (2, 3, 5, 64)])
def test_f32_doubly_kmajor_scalar_tail(gpu_device, M, N, K, bm):
    """Both operands k-major with M, N and K no multiples of 4: the last float4 of a k-row takes load_kmajor's scalar tail (NaN behind it)."""
    _f32_case("kk", 1, M, N, K, pad=0, want_bm=bm)
    _f32_case("kk", 1, M, N, K, pad=4, want_bm=bm)


@gpu
@pytest.mark.parametrize("layout", ["nt", "nk", "kk"])
@pytest.mark.parametrize("M,N", [(1, 1), (1, 65), (127, 63), (128, 64), (129, 65), (129, 1)])
def test_f32_edges(gpu_device, M, N, layout):
    _f32_case(layout, 1, M, N, 36, pad=0, want_bm=64)
    _f32_case(layout, 1, M, N, 36, pad=8, want_bm=64, scale=0.37)


@gpu
@pytest.mark.parametrize("layout", ["nt", "nk", "kk"])
@pytest.mark.parametrize("Z,M,N,bm", [(15, 1100, 520, 128), (16, 1000, 440, 64), (3, 130, 97, 64)])
def test_f32_batched(gpu_device, Z, M, N, bm, layout):
    """Uniform batches run as ONE 1-D grid over batch x tiles_m virtual M-tiles: 9 x 15 = 135 (padded to 136 block rows), 16 x 16, 3 x 3 = 9
    (padded to 16: the workgroups past the batch return).  All three batch strides are larger than the matrices, NaN in between."""
    _f32_case(layout, Z, M, N, 36, pad=4, want_bm=bm, scale=1.0 if layout == "nt" else 0.37)


EPILOGUES = ["bias_relu", "bias_sin", "res_ldr", "alpha_mix_scale", "scale", "inplace", "inplace_alpha"]


@gpu
@pytest.mark.parametrize("kind", EPILOGUES)
@pytest.mark.parametrize("tile,M,N", [("short", 300, 200), ("tall", 8065, 1024)])
def test_f32_epilogues(gpu_device, tile, M, N, kind):
    """gemm_f32.hip:209-216 on both tiles: bias + ReLU, bias + sin(30 v) (the Siren encoder), a residual with ldr > N and NaN in its gap,
    the alpha mix with a scale of neither 0 nor 1, the in-place residual (C is res)."""
    K = 36
    A, B, ref, e32, bias, res, alpha = _f32_data(1, M, N, K, 1.0 if kind == "bias_sin" else 3.0)      # |30 v| stays below ~50 for the sine
    kw = {"bias_relu": dict(bias=bias, relu=1), "bias_sin": dict(bias=bias, relu=2), "res_ldr": dict(bias=bias, res=res),
          "alpha_mix_scale": dict(bias=bias, res=res, alpha=alpha, scale=0.25), "scale": dict(scale=1.7),
          "inplace": dict(res=res, inplace=True), "inplace_alpha": dict(bias=bias, res=res, alpha=alpha, scale=1.7, inplace=True)}[kind]
    want = expected_f32(M, N, K)
    assert want.startswith("gemm_nt_f32_kernel<128" if tile == "tall" else "gemm_nt_f32_kernel<64"), want
    got, inst = _run_f32("nt", A, B, 4, **kw)
    assert inst == {want}, (inst, want)
    kw.pop("inplace", None)
    want64 = _epilogue64(ref, **kw)
    s = max(kw.get("scale", 1.0), 1.0)            # the product's error passes through the scale
    _check(f"f32 epilogue {kind} {tile} {M}x{N}x{K}", got, want64, _bound(e32 * s, ref, factor=30.0 if kind == "bias_sin" else 1.0))


@gpu
@pytest.mark.parametrize("Z,m,n,D,lds", [(3, 130, 97, 64, 100), (3, 130, 97, 64, 104), (1, 8065, 1021, 36, 1024), (2, 65, 1, 4, 4)])
def test_f32_og_scores(gpu_device, Z, m, n, D, lds):
    """og_scores: S[z] = g0[z] g1[z]^T D^-1/2 into rows of lds >= n floats.  n % 4 != 0: nothing past column (n + 3) / 4 * 4 of a row and
    nothing behind the last matrix may be written."""
    A, B, ref, e32, *_ = _f32_data(Z, m, n, D)
    dev = _dev()
    S = torch.full((Z * m + 2, lds), SENT, device=dev)
    g0, g1 = A.to(dev), B.to(dev)
    inst, _ = _traced(lambda: _lib.call("og_scores", dev, g0.data_ptr(), g1.data_ptr(), Z, m, n, D, S.data_ptr(), lds, _lib.STREAM))
    assert inst == {expected_f32(m, n, D, Z)}, inst
    out = S.cpu()
    assert (out[Z * m:] == SENT).all()
    out = out[:Z * m].view(Z, m, lds)
    assert (out[:, :, _round4(n):] == SENT).all()
    _check(f"og_scores Z={Z} {m}x{n}x{D} lds={lds}", out[:, :, :n], ref * D ** -0.5, _bound(e32 * D ** -0.5, ref))


def _reduce(part, parts, rows, ld, cols, with_db):
    """og_splitk_reduce over part [parts][rows][ld] (device, contiguous) -> (dW [rows, cols], db [rows] or None) on the CPU."""
    dev = _dev()
    assert part.is_contiguous() and part.numel() >= parts * rows * ld and ld >= cols + (4 if with_db else 0)
    dW = torch.full((rows + 1, cols), SENT, device=dev)
    db = torch.full((rows + 4,), SENT, device=dev) if with_db else None
    _lib.call("og_splitk_reduce", dev, part.data_ptr(), parts, rows, ld, cols, dW.data_ptr(), _lib.ptr(db), _lib.STREAM)
    dW = dW.cpu()
    assert (dW[rows:] == SENT).all()
    if with_db:
        db = db.cpu()
        assert (db[rows:] == SENT).all()
        db = db[:rows]
    return dW[:rows], db


def _check_reduce(tag, part_cpu, dW, db, cols):
    """dW / db against the float64 sum of the partial products they were reduced from; e32: the CPU fp32 sum of the same terms."""
    part_cpu = part_cpu[:, :, :cols + 1]
    ref = part_cpu.double().sum(0)
    e32 = (part_cpu.sum(0).double() - ref).abs().max().item()
    _check(f"{tag} dW", dW, ref[:, :cols], _bound(e32, ref))
    if db is not None:
        _check(f"{tag} db", db, ref[:, cols], _bound(e32, ref))


@gpu
@pytest.mark.parametrize("Cout,Cin,Kc,parts,T", [(132, 68, 36, 5, 173), (132, 68, 44, 4, 130), (512, 512, 40, 32, 1267), (512, 512, 40, 33, 1267)])
def test_f32_split_k(gpu_device, Cout, Cin, Kc, parts, T):
    """The weight gradient dW = dz^T x as `parts` problems of one doubly k-major launch (k_total = T) with the column sums of dz in an
    extra output column, on both tiles.  T leaves a ragged last chunk; (44, 4, 130) and (40, 33, 1267) leave the last problem NO rows at
    all: its partial product and column sums must be exactly zero.  Then og_splitk_reduce over the partials."""
    g = torch.Generator().manual_seed(T + Cout)
    dz, x = torch.randn(T, Cout, generator=g), torch.randn(T, Cin, generator=g) * 0.3
    dev = _dev()
    lda, ldb, ldc = Cout + 4, Cin + 8, Cin + 4
    Ad, Bd = _gapped(dz[None], lda, 0, NAN)[0], _gapped(x[None], ldb, 0, NAN)[0]
    part = torch.full((parts * Cout + 2, ldc), SENT, device=dev)
    want = expected_f32(Cout, Cin, Kc, parts, True, True)
    inst, _ = _traced(lambda: _lib.call("og_gemm_kmajor", dev, Ad.data_ptr(), lda, Kc * lda, 1, Bd.data_ptr(), ldb, Kc * ldb, part.data_ptr(), ldc,
                                        Cout * ldc, Cout, Cin, Kc, parts, T, 1, 1.0, _lib.STREAM))
    assert inst == {want}, (inst, want)
    assert want.startswith("gemm_nt_f32_kernel<128" if Cout == 512 else "gemm_nt_f32_kernel<64"), want
    out = part.cpu()
    assert (out[parts * Cout:] == SENT).all()
    out = out[:parts * Cout].view(parts, Cout, ldc)
    assert (out[:, :, Cin + 1:] == SENT).all()                       # the column sums take ONE extra column
    ref = torch.zeros(parts, Cout, Cin + 1, dtype=torch.float64)
    e32 = 0.0
    for z in range(parts):
        a, b = dz[z * Kc:min((z + 1) * Kc, T)], x[z * Kc:min((z + 1) * Kc, T)]
        if a.shape[0] == 0:
            assert torch.count_nonzero(out[z, :, :Cin + 1]) == 0, "a problem without rows must leave exact zeros"
            continue
        ref[z, :, :Cin] = a.double().T @ b.double()
        ref[z, :, Cin] = a.double().sum(0)
        e32 = max(e32, ((a.T @ b).double() - ref[z, :, :Cin]).abs().max().item(), (a.sum(0).double() - ref[z, :, Cin]).abs().max().item())
    _check(f"split-K partials {Cout}x{Cin} Kc={Kc} parts={parts} T={T} {want}", out[:, :, :Cin + 1], ref, _bound(e32, ref))
    dW, db = _reduce(part, parts, Cout, ldc, Cin, True)
    _check_reduce(f"split-K reduce {Cout}x{Cin} parts={parts}", out, dW, db, Cin)
    full = dz.double().T @ x.double()
    e32f = ((dz.T @ x).double() - full).abs().max().item()
    _check(f"split-K dW end to end {Cout}x{Cin} T={T}", dW, full, _bound(e32f, full))


@gpu
@pytest.mark.parametrize("with_db", [True, False])
@pytest.mark.parametrize("parts", [1, 4, 5, 16, 17, 29])
def test_f32_splitk_reduce_loop_ends(gpu_device, parts, with_db):
    """og_splitk_reduce: wave w sums the parts w, w + 4, ... sixteen at a time, then four at a time: 1, 4 and 5 parts end in the 4-wide
    loop, 16 is the most the 16-wide loop does not take, 17 its first round, 29 one round and the longest tail.  37 rows x 17 or 18 float4
    columns leave the last workgroup partly idle."""
    rows, cols, ld = 37, 68, 76
    g = torch.Generator().manual_seed(parts)
    part_cpu = torch.randn(parts, rows, ld, generator=g) * 0.3
    dW, db = _reduce(part_cpu.to(_dev()), parts, rows, ld, cols, with_db)
    _check_reduce(f"splitk_reduce parts={parts} db={with_db}", part_cpu, dW, db, cols)


# ----------------------------------------------------------------------------- 2. split-f16 through the public entries
@functools.lru_cache(maxsize=1)
def _h_data(M, N, K):
    """Operands as the kernel is given them: hl32 rows of a (randn x 3) and of 256 b (randn x 0.05) on the device, their merged values,
    float64 a b^T, e32 of the CPU fp32 product, a bias and a residual (fp32, and as hl32 rows with their merged values)."""
    dev = _dev()
    g = torch.Generator().manual_seed(M * 3 + N * 5 + K)
    a, b = torch.randn(M, K, generator=g) * 3.0, torch.randn(N, K, generator=g) * 0.05
    a_hl, b_hl = ops.split_f16_hl(a.to(dev)), ops.split_f16_hl((b * 256.0).to(dev))
    a_in, b_in = ops.merge_f16_hl(a_hl).cpu(), ops.merge_f16_hl(b_hl).cpu() / 256.0
    prod = a_in.double() @ b_in.double().T
    e32 = ((a_in @ b_in.T).double() - prod).abs().max().item()
    d = dict(a_hl=a_hl, b_hl=b_hl, prod=prod, e32=e32, bias=torch.randn(N, generator=g) * 0.3)
    if N % 32 == 0:
        d["res"] = torch.randn(M, N, generator=g) * 2.0
        d["res_hl"] = ops.split_f16_hl(d["res"].to(dev))
        d["res_in"] = ops.merge_f16_hl(d["res_hl"]).cpu()
    return d


FORMS = {       # name -> (output rows, fp32 output too, relu, residual)
    "relu_hl": ("hl", False, True, None), "reshl_hl": ("hl", False, False, "hl"), "plain_hl": ("hl", False, False, None),
    "relu_reshl_hl": ("hl", False, True, "hl"), "planes": ("planes", False, False, None), "planes_relu": ("planes", False, True, None),
    "c32_hl": ("hl", True, False, None), "res32_hl": ("hl", False, False, "f32"), "c32": (None, True, False, None),
    "c32_relu_res32_planes": ("planes", True, True, "f32"),
}


def _half_gapped(t, ld, extra_rows, fill):
    R, C = t.shape
    buf = torch.full((R + extra_rows, ld), fill, dtype=torch.float16, device=t.device)
    buf[:R, :C] = t
    return buf


def _run_h(d, M, N, K, form, pad, alias=False):
    """One launch of og_gemm_nt_f16x3 / og_gemm_nt_f16x3_reshl.  pad: 64 NaN halves after every operand row and three NaN rows after each
    operand, the outputs in a sentinel (64 halves / 8 floats after every row, three rows after the last).  alias: the hl32 residual lies
    in the output rows (res_hl == Ch, the fc.3 form).  -> dict(merged, c32, raw (the hl32 rows, bit for bit), inst)."""
    out_kind, c32, relu, res = FORMS[form]
    dev = _dev()
    er, hp = (3, 64) if pad else (0, 0)
    lda = 2 * K + hp
    Ab, Bb = (_half_gapped(d["a_hl"], lda, er, NAN), _half_gapped(d["b_hl"], lda, er, NAN)) if pad else (d["a_hl"], d["b_hl"])
    ch = cl = cbuf = None
    ldch, ldc = N, _round4(N) + (8 if pad else 0)
    if out_kind == "hl":
        ldch = 2 * N + hp
        ch = torch.full((M + er, ldch), SENT, dtype=torch.float16, device=dev)
    elif out_kind == "planes":
        ldch = N + hp
        ch, cl = (torch.full((M + er, ldch), SENT, dtype=torch.float16, device=dev) for _ in range(2))
    if c32:
        cbuf = torch.full((M + er, ldc), SENT, device=dev)
    rp, ldr, entry = None, N, "og_gemm_nt_f16x3"
    if res == "f32":
        Rb = _gapped(d["res"][None], N + (4 if pad else 0), 0, NAN)[0]
        rp, ldr = Rb.data_ptr(), Rb.shape[1]
    elif res == "hl":
        entry = "og_gemm_nt_f16x3_reshl"
        if alias:
            assert out_kind == "hl"
            ch[:M, :2 * N] = d["res_hl"]
            rp, ldr = ch.data_ptr(), ldch
        else:
            Rb = _half_gapped(d["res_hl"], 2 * N + hp, 0, NAN)
            rp, ldr = Rb.data_ptr(), Rb.shape[1]
    bias = d["bias"].to(dev) if N % 4 == 0 else None       # N % 4 != 0: the launcher takes a bare fp32 output only
    inst, _ = _traced(lambda: _lib.call(entry, dev, Ab.data_ptr(), lda, Bb.data_ptr(), lda, M, N, K, 1.0 / 256.0, _lib.ptr(bias), int(relu), rp, ldr,
                                        _lib.ptr(cbuf), ldc, _lib.ptr(ch), _lib.ptr(cl), ldch, int(out_kind == "hl"), _lib.STREAM))
    tag = f"f16x3 {form} {M}x{N}x{K}"
    r = dict(inst=inst, merged=None, c32=None, raw=None)
    if out_kind == "hl":
        _untouched(tag, ch, M, 2 * N)
        r["raw"] = ch[:M, :2 * N].contiguous()
        r["merged"] = ops.merge_f16_hl(r["raw"]).cpu()
    elif out_kind == "planes":
        _untouched(tag, ch, M, N)
        _untouched(tag, cl, M, N)
        r["merged"] = ops.merge_f16(ch[:M, :N], cl[:M, :N]).cpu()
    if c32:
        _untouched(tag, cbuf, M, _round4(N))          # N % 4 != 0: the last float4 of a row may spill into the padding up to (N + 3) / 4 * 4
        r["c32"] = cbuf[:M, :N].cpu()
    return r


def _h_ref(d, form):
    _, _, relu, res = FORMS[form]
    v = d["prod"] + d["bias"].double() if d["prod"].shape[1] % 4 == 0 else d["prod"]
    if relu:
        v = torch.relu(v)
    if res == "hl":
        v = v + d["res_in"].double()
    elif res == "f32":
        v = v + d["res"].double()
    return v


def _h_case(M, N, K, form, pad, want=None):
    d = _h_data(M, N, K)
    out_kind, c32, relu, res = FORMS[form]
    pred = expected_f16x3(M, N, K, c32=c32, planes=out_kind == "planes", hl=out_kind == "hl", relu=relu, res32=res == "f32", res_hl=res == "hl")
    if want is not None:
        assert pred == want, (pred, want)
    r = _run_h(d, M, N, K, form, pad)
    assert r["inst"] == {pred}, (r["inst"], pred)
    ref = _h_ref(d, form)
    tag = f"f16x3 {form} {M}x{N}x{K} pad={int(pad)} {pred}"
    if r["merged"] is not None:
        _check(tag, r["merged"], ref, _bound(d["e32"], ref, hl=True))
    if r["c32"] is not None:
        _check(tag + " fp32", r["c32"], ref, _bound(d["e32"], ref))
    return r


BIG2 = {"relu_hl": "<1, 2>", "reshl_hl": "<1, 3>", "plain_hl": "<1, 1>", "relu_reshl_hl": "<1, 0>", "res32_hl": "<1, 0>", "planes": "<2, 1>",
        "planes_relu": "<2, 0>", "c32_hl": "<0, 0>"}


# 48 x 4 = 192 tiles at three k-steps; 192 x 1: a one-column grid; 50 x 4: tiles_m no multiple of 8, so the block ids are padded to 56 rows
@gpu
@pytest.mark.parametrize("form", list(BIG2))
@pytest.mark.parametrize("M,N,K,pad", [(12288, 1024, 96, True), (49152, 256, 32, False), (12800, 1024, 32, True)])
def test_f16x3_big2_epilogues(gpu_device, M, N, K, pad, form):
    """The seven epilogue instances of the second-generation 256-tile kernel, each on every grid, float64 on the whole output: the block-id
    remap (eight M-tiles per XCD round) sends most workgroups to rows a first / last slice never sees."""
    _h_case(M, N, K, form, pad, want=f"gemm_nt_f16x3_big2_kernel{BIG2[form]}")


@gpu
@pytest.mark.parametrize("form", ["relu_hl", "reshl_hl", "planes_relu"])
def test_f16x3_big2_partial_last_tile(gpu_device, form):
    """M = 12288 - 5: still 48 x 4 tiles, the last M-tile five rows short -> the run-time instance with predicated stores."""
    _h_case(12288 - 5, 1024, 96, form, True, want="gemm_nt_f16x3_big2_kernel<0, 0>")


T128 = {"relu_hl": "1, 2", "plain_hl": "1, 1", "reshl_hl": "1, 3", "planes": "2, 1"}


@gpu
@pytest.mark.parametrize("form", list(T128))
def test_f16x3_191_tiles_fall_back(gpu_device, form):
    """M = 12288 - 256: 47 x 4 = 188 256-tiles, under the 192 the large tile needs: the 128-tile specialisations take the launch (94 x 8 tiles)."""
    _h_case(12288 - 256, 1024, 96, form, False, want=f"gemm_nt_f16x3_kernel<128, 2, RaggedNone, {T128[form]}>")


@gpu
@pytest.mark.parametrize("pad", [False, True])
@pytest.mark.parametrize("form", list(T128))
def test_f16x3_tile128_whole(gpu_device, form, pad):
    _h_case(256, 256, 96, form, pad, want=f"gemm_nt_f16x3_kernel<128, 2, RaggedNone, {T128[form]}>")


@gpu
@pytest.mark.parametrize("form", ["relu_hl", "relu_reshl_hl", "res32_hl", "c32_hl", "planes_relu", "c32_relu_res32_planes"])
@pytest.mark.parametrize("M,N", [(129, 96), (255, 192), (255, 96), (129, 192)])
def test_f16x3_tile128_generic(gpu_device, M, N, form):
    _h_case(M, N, 96, form, True, want="gemm_nt_f16x3_kernel<128, 2, RaggedNone, 0, 0>")


@gpu
@pytest.mark.parametrize("form", ["relu_reshl_hl", "res32_hl", "c32_hl", "planes_relu", "c32_relu_res32_planes"])
def test_f16x3_tile128_whole_tiles_without_a_specialisation(gpu_device, form):
    """Whole 128-tiles whose epilogue is none of the four compile-time forms stay on the generic instance."""
    _h_case(256, 256, 96, form, True, want="gemm_nt_f16x3_kernel<128, 2, RaggedNone, 0, 0>")


@gpu
@pytest.mark.parametrize("M,N,K", [(130, 97, 64), (1, 65, 32), (257, 131, 96)])
def test_f16x3_bare_fp32_odd_n(gpu_device, M, N, K):
    """A bare fp32 output with N % 4 != 0 into rows padded to a multiple of 4 (the score matrix): the last float4 of a row may spill into
    the padding, no further, and rows past M stay."""
    _h_case(M, N, K, "c32", True, want="gemm_nt_f16x3_kernel<128, 2, RaggedNone, 0, 0>")
    _h_case(M, N, K, "c32", False, want="gemm_nt_f16x3_kernel<128, 2, RaggedNone, 0, 0>")


@gpu
@pytest.mark.parametrize("form", ["relu_hl", "reshl_hl", "planes", "c32_hl", "c32_relu_res32_planes"])
@pytest.mark.parametrize("N", [32, 64])
@pytest.mark.parametrize("M", [1, 127, 128, 129])
def test_f16x3_tile64(gpu_device, M, N, form):
    _h_case(M, N, 96, form, True, want="gemm_nt_f16x3_kernel<64, 2, RaggedNone, 0, 0>")


@gpu
@pytest.mark.parametrize("M,N,K,want", [(12288, 1024, 96, "gemm_nt_f16x3_big2_kernel<1, 3>"), (12288 - 5, 1024, 96, "gemm_nt_f16x3_big2_kernel<0, 0>"),
                                        (256, 256, 96, "gemm_nt_f16x3_kernel<128, 2, RaggedNone, 1, 3>"),
                                        (255, 192, 96, "gemm_nt_f16x3_kernel<128, 2, RaggedNone, 0, 0>"),
                                        (129, 64, 96, "gemm_nt_f16x3_kernel<64, 2, RaggedNone, 0, 0>")])
def test_f16x3_residual_aliases_output(gpu_device, M, N, K, want):
    """res_hl == Ch (the fc.3 form: the residual stream is updated in place; include/openglue_amd.h allows it), on the specialised and on
    the run-time instances: bit for bit the rows of the call with the residual elsewhere."""
    r = _h_case(M, N, K, "reshl_hl", True, want=want)
    a = _run_h(_h_data(M, N, K), M, N, K, "reshl_hl", True, alias=True)
    assert a["inst"] == {want}, a["inst"]
    assert torch.equal(a["raw"], r["raw"]), "the in-place residual changed the result"


# ----------------------------------------------------------------------------- 3. the forms only og_forward / og_forward_ragged launch
TOL_SINKHORN = 1e-4          # tests/test_gpu_parity.py: test_sinkhorn_vs_oracle
TOL_TAP = 1e-4               # tests/test_gpu_parity.py: test_stage_taps_against_reference_layers (x scale)
GENERIC128 = "gemm_nt_f16x3_kernel<128, 2, RaggedNone, 0, 0>"


def _model(D=256, stages=1, residual=True, iters=2, zero_fc3=False):
    from tests.test_gpu_parity import _build
    cfg = syn.make_config(descriptor_dim=D, num_stages=stages, num_heads=4, num_iters=iters, side_info_size=1, residual=residual)
    sd = syn.make_state_dict(cfg, seed=0)
    if zero_fc3:             # x + fc(...) = x: the residual stream leaves the GNN as the keypoint encoder wrote it, whatever kernels ran in between
        for k in sd:
            if k.startswith("attention_gnn.") and ".fc.3." in k:
                sd[k] = torch.zeros_like(sd[k])
    return cfg, sd, _build(cfg, sd, _dev())


def _no_grad(fn):
    with torch.no_grad():
        return fn()


def _projection64(x, desc, sd, cfg):
    """superglue.py:58-62 in float64 and in fp32 on the CPU: -> (g [.., n, D] float64, e32)."""
    def run(dt):
        g = orc.conv1x1(x.to(dt), sd, "linear_proj")
        if cfg.get("residual", False):
            al = torch.sigmoid(orc._w(sd, "mix_coefs", dt)[:, 0])
            g = al * g + (1.0 - al) * desc.to(dt)
        return g
    g64 = run(torch.float64)
    return g64, (run(torch.float32).double() - g64).abs().max().item()


def _scores64(ctx0, ctx1, sd, cfg):
    """The float64 oracle on context descriptors [B, D, m], [B, D, n] as returned: g0 g1^T D^-1/2, then Sinkhorn with dustbins."""
    D = cfg["descriptor_dim"]
    S = (ctx0.double().transpose(1, 2) @ ctx1.double()) * D ** -0.5
    return orc.matching_log_probs(S, orc._w(sd, "dustbin_score", torch.float64), cfg["otp"]["num_iters"], cfg["otp"]["reg"])


@gpu
@pytest.mark.parametrize("residual", [True, False])
@pytest.mark.parametrize("B,m,n", [(1, 130, 97), (3, 130, 97), (3, 300, 257)])
def test_forward_final_projection(gpu_device, B, m, n, residual):
    """The final projection (api.hip: forward_impl): alpha + Ct with residual=True, Ct alone without.  x: the residual stream at the last tap
    (the (hi, lo) rows the launch reads, merged); the returned context descriptors are channel-first, so this checks the transposed store.
    Then the score launch of the same call (one pair: batch = 0; three pairs: a batched launch on the 128 tile) from those descriptors."""
    cfg, sd, model = _model(residual=residual)
    data = syn.make_batch(B, m, n, 256, 1, seed=11 + B)
    dd = to_device(data, _dev())
    x0, x1 = model.forward_tap(dd, 2)
    box = []
    inst, _ = _traced(lambda: box.append(_no_grad(lambda: model(dd))))
    out = {k: v.cpu() for k, v in box[0].items()}
    assert expected_f16x3(B * m, 256, 256, hl=True, res32=residual, alpha=residual, ct=True) == GENERIC128
    assert expected_f16x3(m, n, 256, batch=B if B > 1 else 0, c32=True) == GENERIC128
    assert GENERIC128 in inst, inst
    for side, x, cnt in ((0, x0, m), (1, x1, n)):
        g64, e32 = _projection64(x.cpu(), data[f"local_descriptors{side}"], sd, cfg)
        _check(f"final projection residual={residual} B={B} side {side} ({cnt} rows)", out[f"context_descriptors{side}"],
               g64.transpose(1, 2), _bound(e32, g64))
    ref = _scores64(out["context_descriptors0"], out["context_descriptors1"], sd, cfg)
    _check(f"scores from context descriptors B={B} {m}x{n}", out["scores"], ref, TOL_SINKHORN)


RAGGED_LENS = [(130, 97), (77, 300), (257, 64), (1, 129)]


def _ragged_pairs(lens, D, seed):
    cpu = []
    for i, (m, n) in enumerate(lens):
        p = syn.make_pair(m, n, D, 1, seed=seed + i)
        p["image0_size"] = list(syn.IMAGE_WH); p["image1_size"] = list(syn.IMAGE_WH)
        cpu.append(p)
    return cpu, [to_device(p, _dev()) for p in cpu]


@gpu
@pytest.mark.parametrize("residual", [True, False])
def test_forward_final_projection_ragged(gpu_device, residual):
    """ct_rag 1 and 2 (og_forward_ragged): the context descriptors of pairs of unequal length come back as packed per-pair [D][m_b] blocks.
    The blocks tile the buffer without a gap, so every element of it is compared.  og_forward_tap has no ragged form; with fc.3 zeroed
    every GNN layer is x + 0, so the x the ragged projection reads is the one the same pair's own single-pair call shows at its last tap."""
    cfg, sd, model = _model(residual=residual, zero_fc3=True)
    cpu, pairs = _ragged_pairs(RAGGED_LENS, 256, 700)
    box = []
    inst, _ = _traced(lambda: box.append(model.match_ragged(pairs, 0.2, context_descriptors=True)))
    want = "gemm_nt_f16x3_kernel<128, 2, RaggedDesc, 0, 0>"
    assert expected_f16x3(sum(m for m, _ in RAGGED_LENS), 256, 256, hl=True, res32=residual, alpha=residual, ct=True, ragged=True) == want
    assert want in inst, inst
    for p, r, (m, n) in zip(cpu, box[0], RAGGED_LENS):
        one = to_device({k: (v[None] if torch.is_tensor(v) else v) for k, v in p.items()}, _dev())
        x0, x1 = model.forward_tap(one, 2)
        for side, x, cnt in ((0, x0, m), (1, x1, n)):
            g64, e32 = _projection64(x.cpu(), p[f"local_descriptors{side}"][None], sd, cfg)
            got = r[f"context_descriptors{side}"].cpu()
            assert got.shape == (256, cnt)
            _check(f"ragged final projection residual={residual} pair {m}x{n} side {side}", got, g64[0].T, _bound(e32, g64))
        ref = _scores64(r["context_descriptors0"].cpu()[None], r["context_descriptors1"].cpu()[None], sd, cfg)
        _check(f"ragged scores from context descriptors pair {m}x{n}", r["scores"].cpu(), ref[0], TOL_SINKHORN)


@gpu
def test_forward_ragged_narrow_scores(gpu_device):
    """Pairs whose second image has at most 64 keypoints: the ragged score launch takes the 64-wide kernel."""
    cfg, sd, model = _model()
    lens = [(130, 60), (77, 64), (5, 1)]
    cpu, pairs = _ragged_pairs(lens, 256, 800)
    box = []
    inst, _ = _traced(lambda: box.append(model.match_ragged(pairs, 0.2, context_descriptors=True)))
    want = "gemm_nt_f16x3_kernel<64, 2, RaggedDesc, 0, 0>"
    assert expected_f16x3(130, 64, 256, batch=3, c32=True, ragged=True) == want
    assert want in inst, inst
    for r, (m, n) in zip(box[0], lens):
        ref = _scores64(r["context_descriptors0"].cpu()[None], r["context_descriptors1"].cpu()[None], sd, cfg)
        _check(f"ragged narrow scores pair {m}x{n}", r["scores"].cpu(), ref[0], TOL_SINKHORN)


@gpu
def test_forward_scores_big_batch(gpu_device):
    """B = 3, m = n = 2048: 8 x 8 x 3 = 192 256-tiles -> the batched score launch runs on big_kernel<RaggedNone> (two Sinkhorn iterations)."""
    cfg, sd, model = _model()
    dd = to_device(syn.make_batch(3, 2048, 2048, 256, 1, seed=21), _dev())
    box = []
    inst, _ = _traced(lambda: box.append(_no_grad(lambda: model(dd))))
    want = "gemm_nt_f16x3_big_kernel<RaggedNone>"
    assert expected_f16x3(2048, 2048, 256, batch=3, c32=True) == want
    assert want in inst, inst
    out = {k: v.cpu() for k, v in box[0].items()}
    del box, dd
    ref = _scores64(out["context_descriptors0"], out["context_descriptors1"], sd, cfg)
    _check("scores from context descriptors B=3 2048x2048 (big_kernel<RaggedNone>)", out["scores"], ref, TOL_SINKHORN)


@gpu
def test_forward_scores_big_batch_ragged(gpu_device):
    """The ragged twin: three pairs of up to 2048 x 2048 keypoints on big_kernel<RaggedDesc>; the smaller pairs leave whole tiles empty."""
    cfg, sd, model = _model()
    lens = [(2048, 2048), (1900, 2048), (2048, 1777)]
    cpu, pairs = _ragged_pairs(lens, 256, 900)
    box = []
    inst, _ = _traced(lambda: box.append(model.match_ragged(pairs, 0.2, context_descriptors=True)))
    want = "gemm_nt_f16x3_big_kernel<RaggedDesc>"
    assert expected_f16x3(2048, 2048, 256, batch=3, c32=True, ragged=True) == want
    assert want in inst, inst
    for r, (m, n) in zip(box[0], lens):
        assert r["scores"].shape == (m + 1, n + 1)
        ref = _scores64(r["context_descriptors0"].cpu()[None], r["context_descriptors1"].cpu()[None], sd, cfg)
        _check(f"ragged scores pair {m}x{n} (big_kernel<RaggedDesc>)", r["scores"].cpu(), ref[0], TOL_SINKHORN)


@gpu
def test_forward_cross_layer_row_split(gpu_device):
    """The row-split launch of a cross layer (api.hip: forward_impl): k | v | q of image 1 and the q of image 0 in ONE 256-tile launch whose rows
    below T0 stop after the q columns.  It needs T0 and T multiples of 256, more than 8192 rows (below, proj_small takes the launch; the
    stream kernel only at D = 128) and at least 192 blocks: B = 2, m = 128, n = 8192 gives T0 = 256, T = 16640, 1 + 64 x 3 = 193 blocks.
    The launch is big2<2, 1> like the self layer's; that it was ONE launch shows in the kernel list: two 256-tile launches per stage and a
    single proj_small launch (the k | v of the updated image 0).  x at tap 2 against float64 of the whole cross layer from x at tap 1."""
    B, m, n, H = 2, 128, 8192, 4
    cfg, sd, model = _model()
    data = syn.make_batch(B, m, n, 256, 1, seed=31)
    dd = to_device(data, _dev())
    x0, x1 = (t.cpu() for t in model.forward_tap(dd, 1))
    box = []
    inst, names = _traced(lambda: box.append(model.forward_tap(dd, 2)))
    y0, y1 = (t.cpu() for t in box[0])
    want = "gemm_nt_f16x3_big2_kernel<2, 1>"
    assert expected_f16x3(B * (m + n), 768, 256, planes=True) == want
    assert names.count(want) == 2, [k for k in names if k.startswith("gemm_nt_f16x3")]
    assert sum(k.startswith("proj_small_kernel") for k in names) == 1, names
    pc = "attention_gnn.layers.1.module"
    with torch.no_grad():
        r0 = orc.message_passing(x0.double(), x1.double(), sd, pc, H, False)
        r1 = orc.message_passing(x1.double(), r0, sd, pc, H, False)
    scale = max(1.0, r0.abs().max().item(), r1.abs().max().item())
    _check(f"row-split cross layer image 0 ({B} x {m})", y0, r0, TOL_TAP * scale)
    _check(f"row-split cross layer image 1 ({B} x {n})", y1, r1, TOL_TAP * scale)
