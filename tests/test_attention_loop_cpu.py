"""The steady-state tile loop of attention_dma_kernel carries no address arithmetic and stays inside its VALU budget (no GPU needed).

Beside a busy matrix pipe a wave gets a vector-ALU issue slot only every ~14 cycles (profiles/r04_probe_mfma_valu_classes.log), so every
vector instruction in the loop that the result does not need costs matrix time.  attention.hip is compiled for gfx950 to assembly with the
library's own flags (scripts/asm_audit.py: the same command as openglue_amd/build.py plus -S) and the basic blocks the compiler annotates
as in-loop are counted by opcode, for the default dh = 64 batch instance and the dh = 32 one:

  * NO in-loop block -- the tile loop, the rescale loops inside it, the same loops of the tiles around it -- holds 64-bit or integer
    address arithmetic (v_lshl_add_u64, v_mad_u64_u32, v_lshlrev_b64, v_mul_lo_u32, v_min_i32): the K/V DMA is addressed by scalar plane
    bases and loop-invariant lane offsets, and the row clamp of a last tile is made outside the loop;
  * the tile loop is the one loop that holds MFMAs: two tile bodies, 96 MFMAs at dh = 64 (48 at dh = 32: half the channels and half the
    dv blocks, the same 64 keys x 32 queries per wave and so the same softmax);
  * the VALU instructions of its fast path number <= 2 x 116 + 16: 116 per tile is the softmax arithmetic the result needs (32 v_exp_f32,
    35 v_add_f32, 48 for the (hi, lo) split, one compare), 16 is slack for compares and moves.  Before the scalar addressing: ~350.

The fast path is the tile loop without its rescale blocks.  A rescale block is one that holds v_max* / v_sub_f32 / v_mul_f32 -- the tile
maximum, s -= delta, O *= alpha: the fast path has none of the three.  A block wrongly taken for fast-path only raises the count.
"""
import collections
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORBIDDEN = ("v_lshl_add_u64", "v_mad_u64_u32", "v_lshlrev_b64", "v_mul_lo_u32", "v_min_i32")
RESCALE_ONLY = ("v_max", "v_sub_f32", "v_mul_f32")
SOFTMAX_VALU_PER_TILE, SLACK = 116, 16


def _audit():
    spec = importlib.util.spec_from_file_location("og_asm_audit", os.path.join(ROOT, "scripts", "asm_audit.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def compiled(tmp_path_factory):
    audit = _audit()
    out = str(tmp_path_factory.mktemp("attention_asm") / "attention.s")
    audit.compile_asm("attention.hip", out)
    asm = open(out).read()
    return audit, asm, audit.kernels(asm)


def _blocks(compiled, dh):
    audit, asm, ks = compiled
    hits = [k for k in ks if f"attention_dma_kernel<{dh}, RaggedNone, 1, 1, 0, 0>" in k]
    assert len(hits) == 1, sorted(ks)
    return audit, audit.parse(asm, ks[hits[0]])


@pytest.mark.parametrize("dh,mfmas", [(64, 96), (32, 48)])
def test_tile_loop_has_no_address_arithmetic_and_keeps_its_valu_budget(compiled, dh, mfmas):
    audit, blocks = _blocks(compiled, dh)
    in_loop = [b for b in blocks if b.in_loop]
    assert in_loop, "the compiler marked no block as in-loop"
    bad = {b.name: {op: n for op, n in b.ops.items() if op.startswith(FORBIDDEN)} for b in in_loop}
    bad = {k: v for k, v in bad.items() if v}
    assert not bad, f"address arithmetic inside a loop (dh = {dh}): {bad}"

    def n_mfma(bs):
        return sum(n for b in bs for op, n in b.ops.items() if audit.classify(op) == "MFMA")
    loops = sorted({b.loop for b in in_loop if n_mfma([b])})
    assert len(loops) == 1, f"expected ONE loop with MFMAs (the tile loop), found {loops}"
    tile_loop = [b for b in in_loop if b.loop == loops[0]]
    assert n_mfma(tile_loop) == mfmas, (n_mfma(tile_loop), mfmas)
    fast = [b for b in tile_loop if not any(op.startswith(RESCALE_ONLY) for op in b.ops)]
    valu = sum((collections.Counter({op: n for op, n in b.ops.items() if audit.classify(op) == "VALU"}) for b in fast), collections.Counter())
    total, budget = sum(valu.values()), 2 * SOFTMAX_VALU_PER_TILE + SLACK
    per_block = {b.name: sum(n for op, n in b.ops.items() if audit.classify(op) == "VALU") for b in fast}
    print(f"[attention loop dh={dh}] fast-path VALU {total} per {mfmas} MFMAs (budget {budget}): {dict(valu)}")
    assert total <= budget, f"dh = {dh}: {total} VALU on the fast path of two tiles (budget {budget}): {dict(valu)}; per block {per_block}"
    assert valu["v_exp_f32_e32"] == 64, dict(valu)            # the count is of the right blocks: two tiles' exponentials, once each
