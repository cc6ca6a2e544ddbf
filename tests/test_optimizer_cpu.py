"""CPU checks of the fused optimizer step (openglue_amd.optim, og_adam_layout / og_adam_step): the float64 restatement in
tests/optimizer_ref.py against torch's own clip_grad_norm_ + Adam + StepLR in float64, the layout algebra, the refusals and the ABI.
No kernel is launched here."""
import ctypes as C
import os
import re

import pytest
import torch

from openglue_amd import _lib
from tests import optimizer_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LR, GAMMA, MAX_NORM = 1e-4, 0.999994, 10.0


def test_restatement_equals_torch_in_float64():
    """clip_grad_norm_ + torch.optim.Adam + StepLR(1, gamma), all float64, over 50 steps against RefAdam: two float64 evaluations of the same
    expressions (only gamma^t against StepLR's chained product differs), so 1e-12 relative.  gamma is far from 1 here so that the
    schedule matters; clipped and unclipped steps both occur."""
    gamma = 0.97
    shapes = [(1,), (3,), (8, 4, 1), (5,), (), (64, 16)]
    g = torch.Generator().manual_seed(5)
    init = [torch.randn(s, generator=g, dtype=torch.float64) for s in shapes]
    params = [torch.nn.Parameter(t.clone()) for t in init]
    opt = torch.optim.Adam(params, lr=LR)
    sched = torch.optim.lr_scheduler.StepLR(opt, step_size=1, gamma=gamma)
    mine = ref.RefAdam([t.clone() for t in init], lr=LR, max_grad_norm=MAX_NORM, scheduler_gamma=gamma)
    numel = sum(t.numel() for t in init)
    clipped = 0
    for scale in ref.gradient_scales(50, numel, seed=1, max_norm=MAX_NORM):
        grads = [scale * torch.randn(s, generator=g, dtype=torch.float64) for s in shapes]
        for p, gr in zip(params, grads):
            p.grad = gr.clone()
        norm = torch.nn.utils.clip_grad_norm_(params, MAX_NORM)
        opt.step()
        sched.step()
        got = mine.step(grads)
        assert abs(got - float(norm)) <= 1e-12 * float(norm)
        clipped += mine.clip_coef < 1.0
    assert 10 <= clipped <= 40, clipped
    assert ref.rel_err([p.detach() for p in params], mine.params) < 1e-12
    assert ref.rel_err([opt.state[p]["exp_avg"] for p in params], mine.exp_avg) < 1e-12
    assert ref.rel_err([opt.state[p]["exp_avg_sq"] for p in params], mine.exp_avg_sq) < 1e-12
    assert mine.steps == 50 and float(opt.state[params[0]]["step"]) == 50
    assert ref.rel_err(torch.tensor(opt.param_groups[0]["lr"]), torch.tensor(LR * gamma ** 50)) < 1e-12


def _layout(numels):
    lib = _lib.load()
    n = len(numels)
    numel = (C.c_int64 * max(n, 1))(*numels)
    offsets = (C.c_int64 * max(n, 1))()
    lay = _lib.og_adam_layout_t()
    rc = lib.og_adam_layout(n, numel, offsets, None, C.byref(lay))
    if rc != 0:
        return rc, None, None, None
    cmap = (C.c_int32 * (2 * lay.num_chunks))()
    assert lib.og_adam_layout(n, numel, offsets, cmap, C.byref(lay)) == 0
    return 0, list(offsets), [(cmap[2 * c], cmap[2 * c + 1]) for c in range(lay.num_chunks)], lay


@pytest.mark.parametrize("case", ["tiny", "C1", "C2"])
def test_layout_algebra(case):
    """Offsets are multiples of 4, segments are disjoint and in order, and the chunk map covers every element of every parameter
    exactly once with chunks that never leave their parameter."""
    numels = [1, 3, 4, 5] if case == "tiny" else ref.parameter_numels(case)
    if case == "C2":
        assert sum(numels) == 11_957_249          # the 256-d, 9-stage model
    rc, offsets, cmap, lay = _layout(numels)
    assert rc == 0
    end = 0
    for off, n in zip(offsets, numels):
        assert off % 4 == 0 and off >= end and off - end < 4
        end = off + n
    assert lay.total == (end + 3) // 4 * 4 and lay.chunk == _lib.OG_ADAM_CHUNK
    assert lay.num_partials == -(-lay.total // _lib.OG_ADAM_NORM_CHUNK)
    assert lay.table_bytes == 24 * len(numels) and lay.workspace_bytes == 8 * (_lib.OG_ADAM_SCALARS + lay.num_partials)
    covered = [0] * len(numels)
    seen = set()
    for t, c in cmap:
        assert 0 <= t < len(numels) and (t, c) not in seen
        seen.add((t, c))
        start = c * lay.chunk
        assert 0 <= start < numels[t]
        covered[t] += min(lay.chunk, numels[t] - start)
    assert covered == numels                       # distinct in-range chunks of one parameter whose sizes add up to numel: each element once
    assert cmap == sorted(cmap)


def test_layout_refuses_empty_and_nonpositive():
    assert _layout([])[0] == -1                    # OG_E_INVALID
    assert _layout([4, 0, 2])[0] == -1
    lib = _lib.load()
    lay = _lib.og_adam_layout_t()
    assert lib.og_adam_layout(1, None, None, None, C.byref(lay)) == -1
    assert lib.og_adam_layout(1, (C.c_int64 * 1)(4), None, None, None) == -1


def test_step_refuses_null_and_misaligned_pointers():
    """og_adam_step checks its arguments before it launches anything: OG_E_INVALID (-1) for null pointers and empty sizes, OG_E_ALIGN (-3)
    for a parameter pointer that is not 16-byte aligned."""
    lib = _lib.load()
    A = 0x10000                                    # never dereferenced: every call below is refused
    ok = (C.c_void_p * 2)(A, A + 64)
    args = lambda **kw: [kw.get("count", 2), kw.get("params", ok), kw.get("table", A), kw.get("cmap", A), kw.get("chunks", 2), kw.get("total", 8),
                         kw.get("grad", A), kw.get("m", A), kw.get("v", A), kw.get("ws", A), 1e-4, 1.0, 0.9, 0.999, 1e-8, 1, 10.0, None]
    assert lib.og_adam_step(*args(params=(C.c_void_p * 2)(A, A + 4))) == -3
    assert lib.og_adam_step(*args(params=(C.c_void_p * 2)(A + 8, A))) == -3
    assert lib.og_adam_step(*args(grad=A + 4)) == -3
    assert lib.og_adam_step(*args(params=(C.c_void_p * 2)(A, None))) == -1
    for key in ("params", "table", "cmap", "grad", "m", "v", "ws"):
        assert lib.og_adam_step(*args(**{key: None})) == -1, key
    for key in ("count", "chunks", "total"):
        assert lib.og_adam_step(*args(**{key: 0})) == -1, key
    assert lib.og_adam_step(*args(total=6)) == -1  # the flat buffers are whole float4s


def test_optimizer_refuses_what_the_reference_does_not_use():
    from openglue_amd.optim import Adam
    p = lambda *shape, **kw: torch.nn.Parameter(torch.zeros(*shape, **kw))
    with pytest.raises(ValueError, match="parameter groups"):
        Adam([{"params": [p(4)]}, {"params": [p(4)]}])
    with pytest.raises(ValueError, match="weight_decay"):
        Adam([{"params": [p(4)], "weight_decay": 0.01}])
    with pytest.raises(ValueError, match="amsgrad"):
        Adam([{"params": [p(4)], "amsgrad": True}])
    with pytest.raises(ValueError, match="maximize"):
        Adam([{"params": [p(4)], "maximize": True}])
    with pytest.raises(ValueError, match="CPU"):
        Adam([p(4)])
    with pytest.raises(ValueError, match="max_grad_norm"):
        Adam([p(4)], max_grad_norm=0.0)
    with pytest.raises(TypeError):
        Adam([p(4)], weight_decay=0.01)            # no such option
    with pytest.raises(ValueError, match="float32"):
        Adam([p(4, dtype=torch.float64)])
    with pytest.raises(ValueError, match="float32"):
        Adam([p(4, dtype=torch.float16)])
    with pytest.raises(ValueError, match="contiguous"):
        Adam([torch.nn.Parameter(torch.zeros(4, 6).t())])
    assert issubclass(Adam, torch.optim.Optimizer)


def test_constructor_signature():
    import inspect
    from openglue_amd import optim
    sig = inspect.signature(optim.Adam.__init__)
    assert list(sig.parameters)[1:] == ["params", "lr", "betas", "eps", "max_grad_norm", "scheduler_gamma"]
    d = {k: v.default for k, v in sig.parameters.items()}
    assert (d["lr"], d["betas"], d["eps"], d["max_grad_norm"], d["scheduler_gamma"]) == (1e-4, (0.9, 0.999), 1e-8, None, 1.0)


def test_abi_version_and_symbol_sets():
    lib = _lib.load()
    assert _lib.OG_ABI_VERSION == 14 and lib.og_abi_version() == 14
    header = open(os.path.join(ROOT, "include", "openglue_amd.h")).read()
    assert re.search(r"#define OG_ABI_VERSION 14\b", header)
    declared = set(re.findall(r"^\s*(?:int|size_t)\s+(og_\w+)\s*\(", header, flags=re.M))
    assert {"og_adam_layout", "og_adam_step"} <= declared
    assert declared == set(_lib.SYMBOLS), declared ^ set(_lib.SYMBOLS)
    for name in declared:
        assert hasattr(lib, name), name
    for name in ("OG_ADAM_CHUNK", "OG_ADAM_NORM_CHUNK", "OG_ADAM_SCALARS", "OG_ADAM_TOTAL_NORM", "OG_ADAM_CLIP_COEF", "OG_ADAM_STEP",
                 "OG_ADAM_LR", "OG_ADAM_STEP_SIZE", "OG_ADAM_INV_SQRT_BC2"):
        assert int(re.search(rf"#define {name}\s+(\d+)", header).group(1)) == getattr(_lib, name), name
    assert C.sizeof(_lib.og_adam_layout_t) == 40
    assert "og_adam" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def test_optimizer_kernels_use_no_scratch(tmp_path):
    """The three kernels compile for gfx950 without scratch or spills (the figures DESIGN.md 4.9 quotes), and the update kernel keeps
    at least two waves per SIMD."""
    import subprocess
    from openglue_amd import build as og_build
    cmd = [og_build._hipcc(), *og_build.FLAGS, "-Rpass-analysis=kernel-resource-usage", "--cuda-device-only", "-c",
           os.path.join(og_build.CSRC, "optimizer.hip"), "-o", str(tmp_path / "k.o")]
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
    for kernel in ("adam_gradnorm_kernel", "adam_prepare_kernel", "adam_update_kernel"):
        hits = [u for k, u in usage.items() if kernel in k]
        assert len(hits) == 1, (kernel, list(usage))
        u = hits[0]
        print(f"{kernel}: SGPRs {u['TotalSGPRs']} VGPRs {u['VGPRs']} scratch {u['ScratchSize [bytes/lane]']} occupancy {u['Occupancy [waves/SIMD]']}")
        assert int(u["ScratchSize [bytes/lane]"]) == 0 and int(u["VGPRs Spill"]) == 0 and int(u["SGPRs Spill"]) == 0, (kernel, u)
        assert int(u["Occupancy [waves/SIMD]"]) >= 2, (kernel, u)
