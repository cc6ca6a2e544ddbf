"""attention = 'linear' (csrc/linear_attention.hip) through the inference path, per kernel instance.

linear_attention_kernel<DH> exists for head sizes 16, 32 and 64; the three differ in how the threads split the kv matrix (PARTS = 16 / 8 / 4,
DVP = 1 / 4 / 16) and in LDS footprint, and the kernel has a branch of its own for token-packed (ragged) batches.  Every case below names
the instance it is meant to run, asserts with the profiler that exactly that one ran (and no softmax attention instance), and compares with
the float64 oracle: scores and context descriptors at the whole-path bar, match indices under the bounded near-tie rule, the residual
stream at every stage boundary."""
import pytest
import torch

from openglue_amd import synthetic as syn
from openglue_amd.kernel_trace import attention_instances, launched_kernels
from oracle import superglue_oracle as orc
from tests.test_gpu_parity import TOL_SCORES, _build, _index_agreement
from tests.util import MATCH_THRESHOLD, to_device

pytestmark = pytest.mark.gpu


def _linear_cfg(D, H, stages, **kw):
    return syn.make_config(descriptor_dim=D, num_stages=stages, num_heads=H, num_iters=6, side_info_size=1, attention="linear", **kw)


def _assert_only_linear(names, dh):
    lin = [k for k in names if k.startswith("linear_attention_kernel<")]
    assert lin and set(lin) == {f"linear_attention_kernel<{dh}>"}, sorted(set(lin))
    assert not attention_instances(names), sorted(attention_instances(names))
    assert not [k for k in names if k.startswith("favor_attention_kernel")]
    return len(lin)


# D, H, m, n, B, stages
CASES = [
    (64, 4, 65, 63, 2, 2),            # <16>, both sides of the 64-row tile
    (128, 8, 129, 2, 2, 2),           # <16>, two keys, three query tiles
    (256, 4, 1024, 1000, 1, 2),       # <64> at the headline width
    (128, 2, 2048, 300, 1, 3),        # <64>, SIFT width, strongly non-square
    (256, 8, 64, 640, 2, 9),          # <32> at 256-d, full depth, exact tile multiples
    (64, 1, 200, 4096, 1, 2),         # <64>, one head, 64 key tiles accumulated in fp32
]


@pytest.mark.parametrize("D,H,m,n,B,stages", CASES)
def test_linear_attention_instances_whole_path(gpu_device, D, H, m, n, B, stages):
    dh = D // H
    cfg = _linear_cfg(D, H, stages)
    sd = syn.make_state_dict(cfg, seed=2)
    model = _build(cfg, sd, gpu_device)
    data = syn.make_batch(B, m, n, D, 1, seed=11)
    dev_data = to_device(data, gpu_device)
    box = {}
    names = launched_kernels(lambda: box.update(out=model.match(dev_data, MATCH_THRESHOLD)))
    launches = _assert_only_linear(names, dh)
    out = {k: v.cpu() for k, v in box["out"].items()}
    ndiff, unexplained, o64 = _index_agreement(out["matches0"], out["scores"], sd, cfg, data)
    err = (out["scores"].double() - o64["scores"]).abs().max().item()
    errc = max((out[k].double() - o64[k]).abs().max().item() for k in ("context_descriptors0", "context_descriptors1"))
    print(f"[linear D={D} H={H} {B}x{m}x{n} L={stages}] linear_attention_kernel<{dh}> x{launches}; scores err {err:.2e}, context err {errc:.2e} "
          f"(tol {TOL_SCORES:.0e}, max |score| {o64['scores'].abs().max().item():.0f}); {ndiff} rows differ, {unexplained} unexplained")
    assert err < TOL_SCORES and errc < TOL_SCORES
    assert unexplained == 0, (ndiff, unexplained)
    # the token-packed launch of the same pairs (per-pair row ranges from the descriptor) = the uniform result, on the same instance
    pairs = []
    for b in range(B):
        p = {k: v[b] for k, v in data.items() if torch.is_tensor(v)}
        p["image0_size"] = data["image0_size"]; p["image1_size"] = data["image1_size"]
        pairs.append(to_device(p, gpu_device))
    names = launched_kernels(lambda: box.update(rag=model.match_ragged(pairs, MATCH_THRESHOLD)))
    _assert_only_linear(names, dh)
    for b, r in enumerate(box["rag"]):
        assert (r["scores"].cpu() - out["scores"][b]).abs().max() < 1e-4
        assert torch.equal(r["matches0"].cpu(), out["matches0"][b])


def test_linear_attention_ragged_pairs_of_different_size(gpu_device):
    """Three pairs of 40 ... 700 keypoints in one token-packed launch (the RaggedDesc branch with per-pair row ranges that differ), each against
    the per-pair float64 oracle."""
    D, H = 256, 4
    cfg = _linear_cfg(D, H, 2)
    sd = syn.make_state_dict(cfg, seed=2)
    model = _build(cfg, sd, gpu_device)
    lens = [(40, 700), (333, 65), (129, 128)]
    pairs_cpu = []
    for i, (m, n) in enumerate(lens):
        p = syn.make_pair(m, n, D, 1, seed=300 + i)
        p["image0_size"] = list(syn.IMAGE_WH); p["image1_size"] = list(syn.IMAGE_WH)
        pairs_cpu.append(p)
    dev_pairs = [to_device(p, gpu_device) for p in pairs_cpu]
    box = {}
    names = launched_kernels(lambda: box.update(res=model.match_ragged(dev_pairs, MATCH_THRESHOLD)))
    _assert_only_linear(names, D // H)
    for p, r, (m, n) in zip(pairs_cpu, box["res"], lens):
        one = {k: (v[None] if torch.is_tensor(v) else v) for k, v in p.items()}
        assert r["scores"].shape == (m + 1, n + 1)
        ndiff, unexplained, o64 = _index_agreement(r["matches0"].cpu()[None], r["scores"].cpu()[None], sd, cfg, one)
        err = (r["scores"].cpu().double() - o64["scores"][0]).abs().max().item()
        print(f"[linear ragged D={D} H={H} {m}x{n}] scores err {err:.2e} (tol {TOL_SCORES:.0e}); {ndiff} rows differ, {unexplained} unexplained")
        assert err < TOL_SCORES
        assert unexplained == 0, (m, n, ndiff, unexplained)


@pytest.mark.parametrize("D,H,m,n,B,stages", [CASES[2], CASES[0]])
def test_linear_attention_stage_taps_against_float64(gpu_device, D, H, m, n, B, stages):
    """The residual stream at every stage boundary: a wrong kv partition in one instance shows at its own tap, not only in the scores."""
    cfg = _linear_cfg(D, H, stages)
    sd = syn.make_state_dict(cfg, seed=2)
    model = _build(cfg, sd, gpu_device)
    data = syn.make_batch(B, m, n, D, 1, seed=11)
    dev_data = to_device(data, gpu_device)
    with torch.no_grad():
        inter = orc.superglue_forward(sd, cfg, data, dtype=torch.float64, return_intermediates=True)["_intermediates"]
    taps = [(inter["x0_in"], inter["x1_in"])] + inter["layer_taps"]
    assert len(taps) == 1 + 2 * stages
    for t, (r0, r1) in enumerate(taps):
        box = {}
        names = launched_kernels(lambda: box.update(x=model.forward_tap(dev_data, t)))
        if t > 0:
            _assert_only_linear(names, D // H)
        x0, x1 = box["x"]
        e = max((x0.cpu().double() - r0).abs().max().item(), (x1.cpu().double() - r1).abs().max().item())
        scale = max(1.0, r0.abs().max().item())
        print(f"[linear D={D} H={H} {B}x{m}x{n}] tap {t}: err {e:.2e} tol {1e-4 * scale:.2e} (|x| max {scale:.1f})")
        assert e < 1e-4 * scale, (t, e)


def test_linear_attention_head_size_128_is_refused_up_front(gpu_device):
    """There is no linear_attention_kernel<128>: og_check_shape refuses the config before anything is enqueued (it used to pass the check and
    fail inside og_forward, after the encoder and the projections)."""
    cfg = _linear_cfg(256, 2, 1)
    model = _build(cfg, syn.make_state_dict(cfg, seed=2), gpu_device)
    data = to_device(syn.make_batch(1, 40, 33, 256, 1, seed=11), gpu_device)
    box = {}

    def run():
        torch.zeros(1, device=gpu_device).add_(1)               # so that the window holds a kernel whatever the library does
        with pytest.raises(RuntimeError, match="og_check_shape: OG_E_SHAPE"):
            model.match(data, MATCH_THRESHOLD)
    names = launched_kernels(run)
    assert not [k for k in names if "og_" in k or "gemm" in k or "encoder" in k or "attention" in k], names
