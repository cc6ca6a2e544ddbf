"""The attention kernels, the training Sinkhorn and linear attention compile without spills and at the occupancy their __launch_bounds__ ask for (no GPU needed).

The hand-placed s_waitcnt and the LDS budgets of csrc/attention.hip assume that every instance keeps its registers and runs the waves per
SIMD its launch bounds promise.  Both files are compiled for gfx950 with the library's own flags (openglue_amd/build.py, per-file flags
included: without -packed-fp32-ops one instance of attention.hip spills), and for every kernel the compiler's resource report must show
ScratchSize 0, no VGPR spill and an occupancy >= ceil(threads x min_blocks / 256) waves per SIMD, with threads and min_blocks read from the
attributes clang writes for __launch_bounds__ ("amdgpu-flat-work-group-size", "amdgpu-waves-per-eu") in the device bitcode.
sinkhorn_train.hip and linear_attention.hip are held to the same: their widest instances (sk_bwd_iter_kernel<65>: a 4096-keypoint training
step; linear_attention_kernel<64>) are the ones a small fixture never launches, and <65> once spilled 274 registers unnoticed.
"""
import math
import os
import re
import shutil
import subprocess

import pytest

from openglue_amd import build as og_build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool(name):
    for c in (shutil.which(name), os.path.join("/opt/rocm/llvm/bin", name)):
        if c and os.path.exists(c):
            return c
    pytest.fail(f"{name} not found")


def _compile(src, tmp_path):
    """-> {mangled kernel: {remark: value}}, {mangled kernel: required waves per SIMD}"""
    cmd = [og_build._hipcc(), *og_build.FLAGS, *og_build.PER_FILE_FLAGS.get(src, []), "-Rpass-analysis=kernel-resource-usage", "--cuda-device-only",
           "-save-temps", "-c", os.path.join(og_build.CSRC, src), "-o", str(tmp_path / "k.o")]
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=tmp_path)
    assert r.returncode == 0, r.stderr[-3000:]
    usage, name = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            usage[name] = {}
            continue
        m = re.search(r":\s{2,}([A-Za-z][^:]*): (\S+) \[-Rpass-analysis", line)
        if m and name:
            usage[name][m.group(1).strip()] = m.group(2)
    bc = [f for f in os.listdir(tmp_path) if f.endswith("gfx950.bc")]
    assert len(bc) == 1, os.listdir(tmp_path)
    ll = subprocess.run([_tool("llvm-dis"), str(tmp_path / bc[0]), "-o", "-"], capture_output=True, text=True, check=True).stdout
    groups = {m.group(1): m.group(2) for m in re.finditer(r"^attributes #(\d+) = \{(.*)\}$", ll, re.M)}
    need = {}
    for m in re.finditer(r"^define [^@]*amdgpu_kernel [^@]*@(\S+?)\(.*\) #(\d+)", ll, re.M):
        attrs = groups[m.group(2)]
        flat = re.search(r'"amdgpu-flat-work-group-size"="\d+,(\d+)"', attrs)
        blocks = re.search(r'"amdgpu-waves-per-eu"="(\d+)', attrs)           # clang records __launch_bounds__'s min blocks here
        assert flat, (m.group(1), attrs)
        need[m.group(1)] = math.ceil(int(flat.group(1)) * (int(blocks.group(1)) if blocks else 1) / 256)
    return usage, need


@pytest.mark.parametrize("src,n_kernels", [("attention.hip", 32), ("attention_train.hip", 7), ("sinkhorn_train.hip", 8), ("linear_attention.hip", 4)])
def test_kernels_do_not_spill_and_reach_their_occupancy(tmp_path, src, n_kernels):
    usage, need = _compile(src, tmp_path)
    assert len(usage) == n_kernels, sorted(usage)
    assert set(need) == set(usage), (sorted(need), sorted(usage))
    bad = []
    for k, u in sorted(usage.items()):
        occ = int(u["Occupancy [waves/SIMD]"])
        print(f"{k}: VGPRs {u['VGPRs']} AGPRs {u['AGPRs']} scratch {u['ScratchSize [bytes/lane]']} spill {u['VGPRs Spill']} occupancy {occ} >= {need[k]}")
        if int(u["ScratchSize [bytes/lane]"]) != 0 or int(u["VGPRs Spill"]) != 0 or occ < need[k]:
            bad.append((k, u, need[k]))
    assert not bad, bad
