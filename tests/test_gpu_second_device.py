"""Tensors on a device that is NOT the current one: every launch must run on that device's stream under that device's context
(openglue_amd/_lib.py: call).  With cuda:0 current and the inputs on cuda:1, each entry is compared bit for bit with the same call on
cuda:0 -- all of these kernels are deterministic, so equality is exact.  Needs two visible GPUs."""
import pytest
import torch

from openglue_amd import features, ops, synthetic as syn
from openglue_amd.superpoint import SuperPointNet

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs two visible GPUs")]
DEVICES = ("cuda:0", "cuda:1")          # the device every call is compared against, the device that is not current


def _randn(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def _same_on_both(fn, *host_inputs):
    """fn(*inputs on dev) -> tensor, tuple or dict of tensors; run on cuda:0 then on cuda:1, cuda:0 being current both times."""
    assert torch.cuda.current_device() == 0
    got = []
    for dev in DEVICES:
        out = fn(*[t.to(dev) for t in host_inputs])
        out = list(out.values()) if isinstance(out, dict) else list(out) if isinstance(out, (tuple, list)) else [out]
        assert all(t.device == torch.device(dev) for t in out)
        torch.cuda.synchronize(dev)
        got.append([t.cpu() for t in out])
    assert torch.cuda.current_device() == 0
    assert len(got[0]) == len(got[1]) and all(torch.equal(a, b) for a, b in zip(*got))


def test_gemm_nt():
    _same_on_both(lambda a, b, bias: ops.gemm_nt(a, b, bias, relu=True), _randn(300, 64, seed=0), _randn(96, 64, seed=1), _randn(96, seed=2))


def test_attention():
    q, k, v = (_randn(2, 200, 128, seed=s) for s in (3, 4, 5))
    _same_on_both(lambda q_, k_, v_: ops.attention(q_ * 32 ** -0.5, k_, v_, 4, return_lse=True), q, k, v)


def test_sinkhorn_and_extract_matches():
    S = _randn(2, 150, 170, seed=6)
    _same_on_both(lambda s: ops.sinkhorn(s, 0.7, 20), S)                       # sizes its resident launch from the CURRENT device
    scores = ops.sinkhorn(S.to("cuda:0"), 0.7, 20).cpu()
    _same_on_both(lambda s: ops.extract_matches(s, 0.2), scores)


def test_prepare_features_output():
    lafs, resp, desc = _randn(2, 50, 2, 3, seed=7), torch.rand(2, 50, generator=torch.Generator().manual_seed(8)), _randn(2, 50, 64, seed=9)
    _same_on_both(lambda l, r, d: features.prepare_features_output(l, r, d, method="affine", log_response=True), lafs, resp, desc)


def test_superpoint_dense():
    sd = syn.make_superpoint_state_dict(False, seed=1)
    img = torch.cat([syn.make_image(120, 160, seed=100 + i) for i in range(2)])

    def dense(image):
        net = SuperPointNet(keypoint_threshold=0.005)
        net.load_state_dict(sd, strict=True)
        return net.eval().to(image.device).dense(image)

    _same_on_both(dense, img)
