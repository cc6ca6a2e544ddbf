#!/usr/bin/env python3
"""Experiment: where a workgroup of attention_dma_kernel spends its life outside the tile loop (needs the OG_ATTN_TRACE=2 build:
scripts/build_ablation.sh attn_life -DOG_ATTN_TRACE=2; OPENGLUE_AMD_LIB=openglue_amd/lib/libog_attn_life.so; add -DOG_ATTN_TAIL8=1 for the
8-byte store tail).

Every wave stamps s_memtime at entry, in front of tile 0's step, behind the last tile's step, behind its last O store and after vmcnt(0).
The C2 self shape (64 problems x 4 heads, 1024 x 1024: 2048 workgroups, four rounds on 512 slots) and the cross shape (32 problems) run
back to back; the stamps of the last launch are read.  Per workgroup the segments are those of its waves' mean and of its last-finishing
wave; the table gives the median over workgroups, in shader cycles and as a share of the wave's life.

    python scripts/trace_attention_tail.py [label]      ->  one markdown table per shape on stdout
"""
import ctypes as C, os, sys, numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from openglue_amd import _lib, ops
label = sys.argv[1] if len(sys.argv) > 1 else os.path.basename(_lib.LIB_PATH)
lib = _lib.load(); dev = torch.device("cuda:0")
lib.og_debug_attn_life.restype = C.c_int
lib.og_debug_attn_life.argtypes = [C.c_void_p, C.c_size_t]
n, D, H, LIFE_WG = 1024, 256, 4, 2048
SEGS = ("entry -> tile 0", "tile 0 -> last tile done", "last tile done -> last O store issued", "last O store issued -> stores complete")
for shape, Z in (("self", 64), ("cross", 32)):
    g = torch.Generator().manual_seed(0)
    q, k, v = [(torch.randn(Z, n, D, generator=g) * s).to(dev) for s in (0.5, 2.0, 2.0)]
    (qh, ql), (kh, kl), (vh, vl) = ops.split_f16(q), ops.split_f16(k), ops.split_f16(v)
    oh = torch.empty(Z, n, D, device=dev, dtype=torch.float16); ol = torch.empty_like(oh)
    st = torch.cuda.current_stream().cuda_stream
    def run(): assert lib.og_attention(qh.data_ptr(), ql.data_ptr(), D, kh.data_ptr(), kl.data_ptr(), D, vh.data_ptr(), vl.data_ptr(), D, oh.data_ptr(), ol.data_ptr(), D, Z, n, n, H, D // H, None, st) == 0
    for _ in range(5): run()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(); e0.record()
    for _ in range(20): run()
    e1.record(); torch.cuda.synchronize()
    us = e0.elapsed_time(e1) / 20 * 1e3
    buf = np.zeros((LIFE_WG, 4, 5), np.uint32)
    assert lib.og_debug_attn_life(buf.ctypes.data, buf.nbytes) == 0
    nwg = min(LIFE_WG, Z * H * (n // 128))
    t = buf[:nwg].astype(np.int64)
    seg = (t[..., 1:] - t[..., :-1]) & 0xFFFFFFFF                              # [wg][wave][4 segments]
    life = (t[..., 4] - t[..., 0]) & 0xFFFFFFFF                                # [wg][wave]
    last = np.argmax((t[..., 4] - t[:, :1, 0]) & 0xFFFFFFFF, axis=1)           # the wave of each workgroup that ends last (one CU: one clock)
    seg_last = seg[np.arange(nwg), last]; life_last = life[np.arange(nwg), last]
    print(f"\n**{label}, {shape} shape** ({Z} problems x {H} heads, {n} x {n}, {nwg} workgroups; traced build {us:.1f} us per launch back to back)\n")
    print("| segment | mean of the waves: median cycles | share of life | last-finishing wave: median cycles | share of life |")
    print("|---|---|---|---|---|")
    for i, name in enumerate(SEGS):
        a, b = seg[..., i].mean(1), seg_last[:, i]
        print(f"| {name} | {np.median(a):.0f} | {np.median(a / life.mean(1)) * 100:.1f} % | {np.median(b):.0f} | {np.median(b / life_last) * 100:.1f} % |")
    out = 1.0 - seg[..., 1].mean(1) / life.mean(1)
    print(f"| life | {np.median(life.mean(1)):.0f} | outside the tile steps {np.median(out) * 100:.1f} % | {np.median(life_last):.0f} | outside {np.median(1.0 - seg_last[:, 1] / life_last) * 100:.1f} % |")
