"""Micro-benchmark of the weight-stationary q | k | v projection (csrc/proj_wstat.hip) through og_proj_block at the three launch shapes of
C2 (self, cross step 1 with the row split, cross step 2): 40 back-to-back launches, best of 5, us per launch.

    python scripts/bench_proj_wstat.py [path/to/libopenglue_amd.so]      # e.g. a build of proj_wstat.hip with -DOG_WSTAT_ABL=n
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from openglue_amd import _lib
if len(sys.argv) > 1:
    _lib.LIB_PATH = sys.argv[1]
from openglue_amd import ops
lib = _lib.load()
dev = torch.device("cuda:0")
K, N = 256, 768
g = torch.Generator().manual_seed(1)
w = torch.randn(N, K, generator=g) * 0.06
st = torch.empty(lib.og_proj_block_stream_bytes(N, K), dtype=torch.uint8)
_lib.check(lib.og_proj_block_pack(N, K, w.data_ptr(), st.data_ptr()), "pack")
st = st.to(dev)
bias = (torch.randn(N, generator=g) * 0.3).to(dev)
inv = torch.full((1,), 1.0 / 256.0, device=dev)
M = 65536
X = torch.zeros(M, 4 * K, dtype=torch.float16, device=dev)
X[:, :2 * K] = ops.split_f16_hl((torch.randn(M, K, generator=g) * 2.0).to(dev))
yh = torch.zeros(M, N, dtype=torch.float16, device=dev); yl = torch.zeros_like(yh)
s = torch.cuda.current_stream().cuda_stream
def run(m, split, a, b, r0=0):
    rc = lib.og_proj_block(X.data_ptr() + r0 * 4 * K * 2, 4 * K, m, K, N, st.data_ptr(), bias.data_ptr(), inv.data_ptr(), yh.data_ptr() + r0 * N * 2, yl.data_ptr() + r0 * N * 2, N, split, a[0], a[1], b[0], b[1], s)
    assert rc == 0, rc
out = []
for name, args in (("self", (M, 0, (0, 0), (0, 24))), ("cross1", (M, 32768, (0, 8), (0, 24))), ("cross2", (32768, 0, (0, 0), (8, 24)))):
    for _ in range(20): run(*args)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    best = 1e9
    for rep in range(5):
        e0.record()
        for _ in range(40): run(*args)
        e1.record(); torch.cuda.synchronize()
        best = min(best, e0.elapsed_time(e1) / 40 * 1000)
    out.append(f"{name} {best:.1f}")
print(os.path.basename(_lib.LIB_PATH), " | ".join(out), "us", flush=True)
