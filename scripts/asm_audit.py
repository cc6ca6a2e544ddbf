"""Instruction audit of one kernel instance: compile one .hip of csrc/ to gfx950 assembly with build.py's own flags and count, per basic block,
the MFMA / VALU (by opcode) / SALU / scalar-memory / LDS / vector-memory instructions.  Blocks the compiler annotates as part of a loop are marked.

    python scripts/asm_audit.py attention.hip 'attention_dma_kernel<64, RaggedNone, 1, 1, 0, 0>' [--loop-only] [--asm FILE.s]

The instance is named by a substring of its demangled name (exactly one kernel must match).  Instructions are classified by opcode prefix only.
profiles/attention_valu_audit.md is this script's table for the default attention instance; tests/test_attention_loop_cpu.py uses parse() and
compile_asm() to hold the tile loop to its VALU budget.
"""
from __future__ import annotations

import argparse
import collections
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from openglue_amd import build as og_build  # noqa: E402

CLASSES = ("MFMA", "VALU", "SALU", "SMEM", "LDS", "VMEM")


class Block:
    """name: the block's label; header / depth: the innermost loop the compiler puts it in (None, 0: none); loop: that loop's outermost
    enclosing loop, filled in by parse(); ops: Counter of opcodes"""

    def __init__(self, name):
        self.name, self.header, self.depth, self.parent, self.loop, self.ops = name, None, 0, None, None, collections.Counter()

    @property
    def in_loop(self):
        return self.header is not None


def classify(op: str) -> str | None:
    if op.startswith("v_mfma") or op.startswith("v_smfmac"):
        return "MFMA"
    if op.startswith("v_"):
        return "VALU"
    if op.startswith(("s_load", "s_buffer_load")):
        return "SMEM"
    if op.startswith("s_"):
        return "SALU"
    if op.startswith("ds_"):
        return "LDS"
    if op.startswith(("global_", "buffer_", "flat_", "scratch_")):
        return "VMEM"
    return None


def compile_asm(src: str, out: str) -> None:
    cmd = [og_build._hipcc(), *og_build.FLAGS, *og_build.PER_FILE_FLAGS.get(src, []), "--cuda-device-only", "-S", os.path.join(og_build.CSRC, src), "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError("hipcc failed:\n" + r.stderr[-3000:])


def _cxxfilt() -> str:
    for c in (shutil.which("llvm-cxxfilt"), "/opt/rocm/llvm/bin/llvm-cxxfilt", shutil.which("c++filt")):
        if c and os.path.exists(c):
            return c
    raise RuntimeError("llvm-cxxfilt not found")


def kernels(asm: str) -> dict:
    """-> {demangled name: mangled name} of every kernel (.amdhsa_kernel directive) in the file"""
    mangled = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", asm, re.M)
    out = subprocess.run([_cxxfilt()], input="\n".join(mangled), capture_output=True, text=True, check=True).stdout.split("\n")
    return dict(zip(out, mangled))


def parse(asm: str, mangled: str) -> list:
    """the basic blocks of one function, in file order"""
    lines = asm.split("\n")
    start = next(i for i, l in enumerate(lines) if l.startswith(mangled + ":"))
    blocks, cur = [], None

    def open_block(name, rest):
        nonlocal cur
        cur = Block(name)
        blocks.append(cur)
        note(rest)

    def note(text):                      # the loop comments the assembly printer puts behind a block's label
        if cur is None:
            return
        m = re.search(r"in Loop: Header=(\S+) Depth=(\d+)", text)
        if m:
            cur.header, cur.depth = m.group(1), int(m.group(2))
        m = re.search(r"This (?:Inner )?Loop Header: Depth=(\d+)", text)
        if m:
            cur.header, cur.depth = cur.name.lstrip(".").lstrip("L"), int(m.group(1))
        m = re.search(r"Parent Loop (\S+) Depth=1\b", text)
        if m:
            cur.parent = m.group(1)

    for line in lines[start + 1:]:
        s = line.strip()
        if s.startswith(".Lfunc_end"):
            break
        m = re.match(r"^(\.LBB\d+_\d+):(.*)$", s) or re.match(r"^; (%bb\.\d+):(.*)$", s)
        if m:
            open_block(m.group(1), m.group(2))
            continue
        if not s or s.startswith((";", ".")):
            note(s)
            continue
        if cur is None:
            open_block("entry", "")
        op = s.split()[0]
        if classify(op):
            cur.ops[op] += 1
    outer = {b.header: b.parent or b.header for b in blocks if b.header and b.name.lstrip(".").lstrip("L") == b.header}
    for b in blocks:
        b.loop = outer.get(b.header)
    return blocks


def totals(ops) -> dict:
    t = dict.fromkeys(CLASSES, 0)
    for op, n in ops.items():
        t[classify(op)] += n
    return t


def table(blocks, loop_only=False) -> str:
    rows = ["| block | loop | " + " | ".join(CLASSES) + " | VALU by opcode |", "|---|---|" + "---|" * len(CLASSES) + "---|"]
    for b in blocks:
        if not b.ops or (loop_only and not b.in_loop):
            continue
        t = totals(b.ops)
        valu = ", ".join(f"{n} {op}" for op, n in sorted(b.ops.items(), key=lambda kv: (-kv[1], kv[0])) if classify(op) == "VALU")
        where = "-"
        if b.in_loop:
            where = f"{b.header} depth {b.depth}" + (f" (in {b.loop})" if b.loop != b.header else "")
        rows.append(f"| {b.name} | {where} | " + " | ".join(str(t[c]) for c in CLASSES) + f" | {valu} |")
    for loop in sorted({b.loop for b in blocks if b.in_loop}):
        tl = totals(sum((b.ops for b in blocks if b.loop == loop), collections.Counter()))
        rows.append(f"| **all of loop {loop}** | | " + " | ".join(str(tl[c]) for c in CLASSES) + " | |")
    return "\n".join(rows)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("source", help="file name under openglue_amd/csrc, e.g. attention.hip")
    ap.add_argument("kernel", help="substring of the demangled kernel name")
    ap.add_argument("--loop-only", action="store_true", help="print only the blocks inside loops")
    ap.add_argument("--asm", help="read this assembly file instead of compiling")
    a = ap.parse_args()
    if a.asm:
        asm = open(a.asm).read()
    else:
        with tempfile.TemporaryDirectory() as d:
            compile_asm(a.source, os.path.join(d, "k.s"))
            asm = open(os.path.join(d, "k.s")).read()
    ks = kernels(asm)
    hits = [k for k in ks if a.kernel in k]
    if len(hits) != 1:
        sys.exit(f"{len(hits)} kernels match {a.kernel!r}:\n" + "\n".join(hits or sorted(ks)))
    print(f"`{hits[0]}`\n")
    print(table(parse(asm, ks[hits[0]]), a.loop_only))


if __name__ == "__main__":
    main()
