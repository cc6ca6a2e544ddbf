"""The loops of mlp_fused_kernel and proj_wstat_kernel hold the arithmetic their results need and no bookkeeping (no GPU needed).

Both files are compiled for gfx950 to assembly with the library's own flags (scripts/asm_audit.py, as tests/test_attention_loop_cpu.py
does for attention.hip) and the basic blocks the compiler annotates as in-loop are counted by opcode.

mlp_fused_kernel<256>: the in-loop blocks are the pass loop -- the 8 residual fc.0 stages, the one-stage fc.0 loop, the two peeled fc.0
stages, the 8 fc.3 stages.
  * none holds v_cmp_eq_u32 / v_perm_b32 (the residual's identity fragment is built once at kernel entry and read from LDS) nor
    v_mul_lo_u32 / v_mad_u64_u32 / v_lshl_add_u64 / v_readfirstlane_b32 (DMA sources are scalar pointers advanced by scalar adds);
  * VALU <= 224 + 32: the arithmetic of a pass is the (hi, lo) conversion of its 4 hidden blocks, 4 x 16 accumulator registers = 64
    v_mul_f32 + 64 v_max_f32 + 32 v_cvt_pk_f16_f32 + 64 v_fma_mix{lo,hi}_f16 = 224; 32 is slack for the ring addresses of the
    stages that keep a run-time slot (5 v_add per such hand-over) and the bias addresses of a pass.
mlp_fused_kernel<128> has ONE pass (4 hidden blocks per half), so the compiler sees no pass loop: the only loop left is the one-stage
fc.0 loop, whose result needs no vector arithmetic at all (derived the same way: the conversion sits in the fc.3 stages, which are
straight-line code here).  Budget 0 + 32; and, as it is the same arithmetic as a 256-d pass, the whole kernel in front of the epilogue
holds exactly those 224 conversion instructions -- asserted by opcode.
Both: the blocks behind the last MFMA (partial-sum exchange, epilogue) hold no v_cndmask_b32: which accumulators a wave hands to its
partner is decided by one wave-uniform branch.

proj_wstat_kernel: the one loop with MFMAs is the steady block loop, two 32-token blocks = 96 MFMAs.  No v_mul_lo_u32 / v_mad_u64_u32 /
v_min_i32 / v_lshl_add_u64 in it (scalar DMA and store bases, loop-invariant lane offsets, the row clamp and the row predicate only in
the blocks around the loop); VALU <= 80 + 16: per block 16 v_mul_f32 (times 1 / pre-scale) + 24 for the (hi, lo) split.

All three: no register spill and no scratch in the compiler's resource-usage remarks."""
import collections
import importlib.util
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MLP_FORBIDDEN = ("v_cmp_eq_u32", "v_perm_b32", "v_mul_lo_u32", "v_mad_u64_u32", "v_lshl_add_u64", "v_readfirstlane_b32")
WSTAT_FORBIDDEN = ("v_mul_lo_u32", "v_mad_u64_u32", "v_min_i32", "v_lshl_add_u64")
MLP_ARITH = {"v_mul_f32": 64, "v_max_f32": 64, "v_cvt_pk_f16_f32": 32, "v_fma_mix": 64}      # one pass: 224
MLP_SLACK, WSTAT_ARITH, WSTAT_SLACK = 32, 80, 16


def _audit():
    spec = importlib.util.spec_from_file_location("og_asm_audit", os.path.join(ROOT, "scripts", "asm_audit.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _compile(tmp_path_factory, src):
    """-> (audit module, assembly, {demangled: mangled}, {mangled: {remark: value}})"""
    audit = _audit()
    out = str(tmp_path_factory.mktemp("loops_asm") / (src + ".s"))
    og = audit.og_build
    cmd = [og._hipcc(), *og.FLAGS, *og.PER_FILE_FLAGS.get(src, []), "--cuda-device-only", "-S", "-Rpass-analysis=kernel-resource-usage", os.path.join(og.CSRC, src), "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    usage, cur = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"remark:\s+(?:Function Name: (\S+)|([A-Za-z ]+?)(?: \[[^\]]*\])?: (\S+))", line)
        if m and m.group(1):
            cur = usage.setdefault(m.group(1), {})
        elif m and cur is not None:
            cur[m.group(2).strip()] = m.group(3)
    asm = open(out).read()
    return audit, asm, audit.kernels(asm), usage


@pytest.fixture(scope="module")
def mlp(tmp_path_factory):
    return _compile(tmp_path_factory, "mlp_fused.hip")


@pytest.fixture(scope="module")
def wstat(tmp_path_factory):
    return _compile(tmp_path_factory, "proj_wstat.hip")


def _kernel(compiled, name):
    audit, asm, ks, usage = compiled
    hits = [k for k in ks if name in k]
    assert len(hits) == 1, sorted(ks)
    return audit, audit.parse(asm, ks[hits[0]]), usage[ks[hits[0]]]


def _valu(audit, blocks):
    return sum((collections.Counter({op: n for op, n in b.ops.items() if audit.classify(op) == "VALU"}) for b in blocks), collections.Counter())


def _forbidden(blocks, ops):
    bad = {b.name: {op: n for op, n in b.ops.items() if op.startswith(ops)} for b in blocks}
    return {k: v for k, v in bad.items() if v}


def _no_spill(usage):
    assert usage["VGPRs Spill"] == "0" and usage["SGPRs Spill"] == "0" and usage["ScratchSize"] == "0", usage


@pytest.mark.parametrize("D,arith", [(256, 224), (128, 0)])
def test_mlp_fused_loops(mlp, D, arith):
    audit, blocks, usage = _kernel(mlp, f"mlp_fused_kernel<{D}>")
    _no_spill(usage)
    in_loop = [b for b in blocks if b.in_loop]
    assert in_loop, "the compiler marked no block as in-loop"
    bad = _forbidden(in_loop, MLP_FORBIDDEN)
    assert not bad, f"D = {D}: bookkeeping inside a loop: {bad}"
    valu = _valu(audit, in_loop)
    total = sum(valu.values())
    print(f"[mlp_fused<{D}> loops] VALU {total} (budget {arith} + {MLP_SLACK}): {dict(valu)}")
    assert total <= arith + MLP_SLACK, dict(valu)
    has_mfma = lambda b: any(audit.classify(op) == "MFMA" for op in b.ops)
    last = max(i for i, b in enumerate(blocks) if has_mfma(b))
    head, tail = blocks[:last + 1], blocks[last + 1:]       # tail: the partial-sum exchange and the epilogue
    # the conversion arithmetic is where it is counted: all of it inside the pass loop at 256-d, all of it in front of the epilogue at 128-d
    conv = _valu(audit, in_loop if D == 256 else [b for b in head if has_mfma(b)])
    for op, n in MLP_ARITH.items():
        assert sum(c for o, c in conv.items() if o.startswith(op)) == n, (op, dict(conv))
    assert tail
    sel = {b.name: b.ops["v_cndmask_b32_e32"] + b.ops["v_cndmask_b32_e64"] for b in tail if any(op.startswith("v_cndmask_b32") for op in b.ops)}
    assert not sel, f"D = {D}: element-wise selects in the exchange / epilogue: {sel}"


def test_proj_wstat_loop(wstat):
    audit, blocks, usage = _kernel(wstat, "proj_wstat_kernel")
    _no_spill(usage)
    in_loop = [b for b in blocks if b.in_loop]
    assert in_loop, "the compiler marked no block as in-loop"
    bad = _forbidden(in_loop, WSTAT_FORBIDDEN)
    assert not bad, f"address arithmetic inside a loop: {bad}"

    def n_mfma(bs):
        return sum(n for b in bs for op, n in b.ops.items() if audit.classify(op) == "MFMA")
    loops = sorted({b.loop for b in in_loop if n_mfma([b])})
    assert len(loops) == 1, f"expected ONE loop with MFMAs (the steady block loop), found {loops}"
    loop = [b for b in in_loop if b.loop == loops[0]]
    assert n_mfma(loop) == 96, n_mfma(loop)
    valu = _valu(audit, loop)
    total = sum(valu.values())
    print(f"[proj_wstat loop] VALU {total} per 96 MFMAs (budget {WSTAT_ARITH} + {WSTAT_SLACK}): {dict(valu)}")
    assert total <= WSTAT_ARITH + WSTAT_SLACK, dict(valu)
    assert valu["v_mul_f32"] == 32 and valu["v_cvt_pk_f16_f32"] == 16, dict(valu)      # the count is of the right blocks: two tiles' scale and split
