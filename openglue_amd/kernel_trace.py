"""Which device kernels a piece of host code launched: the names the dispatch tests (tests/test_gpu_attention_dispatch.py, tests/test_gpu_gemm_forms.py, tests/test_gpu_proj_mlp_forms.py,
tests/test_gpu_attention_backward.py, tests/test_gpu_sinkhorn_forms.py, tests/test_gpu_superpoint_train_forms.py, tests/test_gpu_superpoint_bn_train_forms.py) and the form checks (scripts/check_attention_pipe.py) assert on.  It lives in the package, not under tests/, so that the scripts can use it on
their own.

launched_kernels(fn) runs fn() under torch.profiler (ProfilerActivity.CUDA: on ROCm, kineto's roctracer records every dispatched kernel
by its demangled name, the library's own included), synchronises, and returns the names in launch order, shortened to the template:
`void (anonymous namespace)::attention_dma_kernel<64, RaggedNone, 2, 1, 0, 0>(AttnArgs, RaggedNone)` ->
`attention_dma_kernel<64, RaggedNone, 2, 1, 0, 0>`.  A window in which the profiler saw no device kernel at all is an error, not an
empty list: an assertion over the names would then hold vacuously.
"""
import re

import torch

ATTENTION_FORWARD = ("attention_kernel<", "attention_dma_kernel<", "attention_p16_kernel<")
GEMM = ("gemm_nt_f32_kernel<", "gemm_nt_f16x3_kernel<", "gemm_nt_f16x3_big_kernel<", "gemm_nt_f16x3_big2_kernel<")
PROJ_MLP = ("mlp_small_kernel<", "mlp_fused_kernel<", "proj_small_kernel<", "proj_stream_kernel<")
ATTENTION_TRAIN = ("attention_bwd_kernel<", "attention_lse_kernel<", "attention_delta_kernel")     # csrc/attention_train.hip
SINKHORN = ("sinkhorn_sweep_kernel<", "sinkhorn_sweep_fast_kernel<", "sinkhorn_combine_kernel<", "sinkhorn_combine_fast_kernel<", "sinkhorn_scores_kernel<",
            "sinkhorn_resident_kernel<", "sinkhorn_fallback_kernel<")     # csrc/sinkhorn.hip, csrc/sinkhorn_resident.hip: the inference Sinkhorn
SUPERPOINT_TRAIN = ("sp_conv3x3_save_kernel<", "sp_dgrad_kernel<SpPlain,", "sp_wgrad_kernel<SpPlain,", "sp_wgrad1a_kernel<SpPlain>", "sp_reduce_parts_kernel", "sp_describe_bwd_point_kernel",
                    "sp_describe_bwd_cell_kernel", "sp_grad_dump_kernel<SpPlain,")     # csrc/superpoint_train.hip: the SuperPoint fine-tuning kernels (the shared bodies of csrc/og_superpoint_train.h as SpPlain)
SUPERPOINT_BN_TRAIN = ("sp_bn_conv1a_kernel", "sp_bn_conv3x3_kernel<", "sp_bn_stats_finish_kernel", "sp_bn_act_kernel", "sp_bn_cell_tail_kernel", "sp_bn_reduce_kernel<",
                       "sp_bn_reduce_finish_kernel", "sp_dgrad_kernel<SpBn,", "sp_wgrad_kernel<SpBn,", "sp_wgrad1a_kernel<SpBn>", "sp_grad_dump_kernel<SpBn,",
                       "sp_reduce_parts_kernel")     # csrc/superpoint_bn_train.hip: the SuperPointNetBn fine-tuning kernels (the shared bodies as SpBn)
PROJ_WSTAT ="proj_wstat_kernel"       # csrc/proj_wstat.hip: the weight-stationary q | k | v projection of 256-d batches (no template arguments)


def short_name(name: str) -> str:
    """Demangled kernel name -> `kernel<template args>` without return type, namespaces and argument list."""
    if name.startswith("_Z"):          # a tracer that reports mangled names
        import subprocess
        try:
            name = subprocess.run(["c++filt", name], capture_output=True, text=True, check=True).stdout.strip() or name
        except (OSError, subprocess.CalledProcessError):
            pass
    s = name.replace("(anonymous namespace)::", "").strip()
    if s.startswith("void "):
        s = s[5:]
    depth = 0
    for i, c in enumerate(s):          # the argument list is the first '(' outside the template brackets
        if c == "<":
            depth += 1
        elif c == ">":
            depth -= 1
        elif c == "(" and depth == 0:
            s = s[:i]
            break
    s = s.strip()
    j = s.find("<")
    head = s if j < 0 else s[:j]
    return head.split("::")[-1] + ("" if j < 0 else s[j:])


def launched_kernels(fn) -> list:
    """Run fn() and return the shortened names of the device kernels it launched, in launch order."""
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    evs = [e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
    if not evs:
        raise RuntimeError("kernel_trace: the profiler recorded no device kernel in this window -- cannot tell which kernels ran")
    evs.sort(key=lambda e: e.time_range.start)
    return [short_name(e.name) for e in evs if not re.match(r"^(Memcpy|Memset|hipMem)", e.name)]


def attention_instances(names) -> set:
    """The attention forward instances among `names`."""
    return {n for n in names if n.startswith(ATTENTION_FORWARD)}


def gemm_instances(names) -> set:
    """The exact-fp32 and split-f16 GEMM instances (csrc/gemm_f32.hip, csrc/gemm_f16x3.hip) among `names`."""
    return {n for n in names if n.startswith(GEMM)}


def proj_mlp_instances(names) -> list:
    """The message-MLP and q | k | v projection launches (csrc/mlp_fused.hip) among `names`, in launch order, one entry per launch."""
    return [n for n in names if n.startswith(PROJ_MLP)]


def projection_candidates(names) -> list:
    """Every launch among `names` that can be a q | k | v projection or sits between two of them in og_forward's GNN -- the message-MLP and projection
    kernels of csrc/mlp_fused.hip, proj_wstat_kernel, the split-f16 GEMM instances -- in launch order, one entry per launch."""
    return [n for n in names if n.startswith(PROJ_MLP + ("gemm_nt_f16x3_",)) or n == PROJ_WSTAT]


def attention_train_instances(names) -> list:
    """The softmax-attention training launches (csrc/attention_train.hip: backward, row log-sum-exp, delta) among `names`, in launch order."""
    return [n for n in names if n.startswith(ATTENTION_TRAIN)]


def sinkhorn_instances(names) -> list:
    """The inference-Sinkhorn launches (csrc/sinkhorn.hip, csrc/sinkhorn_resident.hip) among `names`, in launch order, one entry per launch."""
    return [n for n in names if n.startswith(SINKHORN)]


def superpoint_train_instances(names) -> list:
    """The SuperPoint fine-tuning launches (csrc/superpoint_train.hip) among `names`, in launch order, one entry per launch."""
    return [n for n in names if n.startswith(SUPERPOINT_TRAIN)]


def superpoint_bn_train_instances(names) -> list:
    """The SuperPointNetBn fine-tuning launches (csrc/superpoint_bn_train.hip) among `names`, in launch order, one entry per launch."""
    return [n for n in names if n.startswith(SUPERPOINT_BN_TRAIN)]
