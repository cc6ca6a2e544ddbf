"""The store tail of attention_dma_kernel exchanges half-waves and stores 16 bytes per lane (no GPU needed).

A lane of the 32x32 MFMA output layout holds four channels of every 8-channel slot of its query row and lane l + 32 the other four, so as 8-byte
stores the tail is 16 store instructions per lane at dh = 64, and it is bound by their issue.  og_attn_store_o (attention.hip) swaps the dwords of
each pair of slots between the half-waves with v_permlane32_swap -- 2 planes x 2 dwords per pair -- and then stores ONE 16-byte run per pair and
plane.  attention.hip is compiled for gfx950 to assembly with the library's own flags (scripts/asm_audit.py, as tests/test_attention_loop_cpu.py
does) and the instructions of the default instances are counted:

  * dh = 64: 4 pairs -> 16 swaps, 8 x 16-byte stores;
  * dh = 32: 2 pairs ->  8 swaps, 4 x 16-byte stores.

The 8-byte stores stay in the kernel as well: they serve an `ldo` that is a multiple of 4 but not of 8 halves.
"""
import collections
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _audit():
    spec = importlib.util.spec_from_file_location("og_asm_audit", os.path.join(ROOT, "scripts", "asm_audit.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def compiled(tmp_path_factory):
    audit = _audit()
    out = str(tmp_path_factory.mktemp("attention_tail_asm") / "attention.s")
    audit.compile_asm("attention.hip", out)
    asm = open(out).read()
    return audit, asm, audit.kernels(asm)


@pytest.mark.parametrize("dh,swaps,wide", [(64, 16, 8), (32, 8, 4)])
def test_store_tail_swaps_half_waves_and_stores_16_bytes(compiled, dh, swaps, wide):
    audit, asm, ks = compiled
    hits = [k for k in ks if f"attention_dma_kernel<{dh}, RaggedNone, 1, 1, 0, 0>" in k]
    assert len(hits) == 1, sorted(ks)
    ops = sum((b.ops for b in audit.parse(asm, ks[hits[0]])), collections.Counter())
    n_swap = sum(n for op, n in ops.items() if op.startswith("v_permlane32_swap"))
    n_wide = sum(n for op, n in ops.items() if op.startswith("global_store_dwordx4"))
    n_narrow = sum(n for op, n in ops.items() if op.startswith("global_store_dwordx2"))
    print(f"[attention store tail dh={dh}] {n_swap} v_permlane32_swap, {n_wide} global_store_dwordx4, {n_narrow} global_store_dwordx2")
    assert n_swap == swaps, (n_swap, swaps)
    assert n_wide >= wide, (n_wide, wide)
