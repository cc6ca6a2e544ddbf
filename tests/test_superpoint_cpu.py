"""SuperPoint without a GPU: the float64 restatement against the reference fixture, the modules' state-dict layouts and loading,
the refusals, and the kernels' compiled resources."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import superpoint_ref as R  # noqa: E402
from test_attention_resources_cpu import _compile  # noqa: E402

from openglue_amd import synthetic as syn  # noqa: E402
from openglue_amd.superpoint import SuperPointNet, SuperPointNetBn, methods  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "superpoint.npz")
EPS = 4e-5      # twice the heatmap bound of tests/test_gpu_superpoint.py


@pytest.mark.parametrize("name", ["sp_b1", "sp_b2", "spbn_b2"])
def test_restatement_matches_reference_fixture(name):
    z = np.load(GOLDEN)
    B, H, W, k, bn = (int(v) for v in z[f"{name}_meta"])
    thr = float(z["threshold"])
    sd = syn.make_superpoint_state_dict(bool(bn), seed=int(z["weight_seed"]))
    img = torch.from_numpy(z[f"{name}_image"]).to(torch.float32) / 255          # 8-bit images, as the generator fed them
    heat, desc = R.dense(sd, img)
    assert (heat - torch.from_numpy(z[f"{name}_heat"]).double()).abs().max() < 5e-6
    sel = R.select(heat, 9, 4, thr, k)
    lafs = torch.from_numpy(z[f"{name}_lafs"])
    assert lafs.shape[1] == len(sel[0]["idx"])
    Wh = heat.shape[2]
    for b, s in enumerate(sel):
        ridx = lafs[b, :, 1, 2].long() * Wh + lafs[b, :, 0, 2].long()
        assert s["order"] == ("raster" if name == "sp_b1" else "desc")
        # the reference run and the float64 selection keep the same keypoints here; in descending order only scores closer than EPS may swap
        assert torch.equal(torch.sort(ridx).values, torch.sort(s["idx"]).values), (name, b)
        s64 = heat[b].flatten()[ridx]
        if s["order"] == "raster":
            assert torch.equal(ridx, s["idx"])
        else:
            assert torch.all(s64[1:] <= s64[:-1] + EPS)
        rows = torch.from_numpy(z[f"{name}_desc_rows"])                          # descriptors are stored for these output rows
        d = R.describe(desc[b], lafs[b, rows, :, 2].double())
        assert (d - torch.from_numpy(z[f"{name}_desc"][b]).double()).abs().max() < 1e-5


@pytest.mark.parametrize("cls", ["SuperPointNet", "SuperPointNetBn"])
def test_state_dict_layout_matches_reference(cls):
    z = np.load(GOLDEN)
    want = [str(s) for s in z[f"layout_{cls}"]]
    got = [f"{k}:{'x'.join(map(str, v.shape))}" for k, v in methods[cls]().state_dict().items()]
    assert got == want


def test_weights_loading(tmp_path):
    sd = syn.make_superpoint_state_dict(False, seed=3)
    torch.save(sd, tmp_path / "sp.pth")
    net = SuperPointNet(weights=tmp_path / "sp.pth")
    assert torch.equal(net.convDb.weight, sd["convDb.weight"])
    # pytorch-superpoint checkpoint: ['model_state_dict'] with its own trunk names
    sdb = syn.make_superpoint_state_dict(True, seed=4)
    inv = {"conv1a": "inc.conv.conv.0", "bn1a": "inc.conv.conv.1", "conv1b": "inc.conv.conv.3", "bn1b": "inc.conv.conv.4"}
    for i in range(1, 4):
        inv.update({f"conv{i + 1}a": f"down{i}.mpconv.1.conv.0", f"bn{i + 1}a": f"down{i}.mpconv.1.conv.1",
                    f"conv{i + 1}b": f"down{i}.mpconv.1.conv.3", f"bn{i + 1}b": f"down{i}.mpconv.1.conv.4"})
    ck = {}
    for key, v in sdb.items():
        mod, rest = key.split(".", 1)
        ck[f"{inv.get(mod, mod)}.{rest}"] = v
    assert any(k.startswith("down3.mpconv") for k in ck)
    torch.save({"model_state_dict": ck}, tmp_path / "spbn.pth.tar")
    netb = SuperPointNetBn(weights=tmp_path / "spbn.pth.tar")
    for key, v in sdb.items():
        assert torch.equal(netb.state_dict()[key], v), key


def test_refusals():
    img = torch.rand(1, 1, 64, 64)
    with pytest.raises(RuntimeError, match="no CPU path"):
        SuperPointNet().eval()(img)
    with pytest.raises(ValueError, match="odd"):
        SuperPointNet(nms_kernel=4)(img)
    with pytest.raises(ValueError, match="256"):
        SuperPointNet(descriptor_dim=128)(img)
    with pytest.raises(NotImplementedError):
        SuperPointNetBn().train()(img)


def test_refuses_images_below_one_cell():
    net = SuperPointNet()
    with pytest.raises(ValueError, match="H // 8"):
        net(torch.empty(1, 1, 7, 64))
    with pytest.raises(ValueError, match="H // 8"):
        net(torch.empty(1, 1, 64, 5))


def test_superpoint_kernels_do_not_spill_and_reach_their_occupancy(tmp_path):
    usage, need = _compile("superpoint.hip", tmp_path)
    assert len(usage) == 11, sorted(usage)
    bad = []
    for k, u in sorted(usage.items()):
        occ = int(u["Occupancy [waves/SIMD]"])
        print(f"{k}: VGPRs {u['VGPRs']} scratch {u['ScratchSize [bytes/lane]']} spill {u['VGPRs Spill']} occupancy {occ} >= {need[k]}")
        if int(u["ScratchSize [bytes/lane]"]) != 0 or int(u["VGPRs Spill"]) != 0 or occ < need[k]:
            bad.append((k, u, need[k]))
    assert not bad, bad
