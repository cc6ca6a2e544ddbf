"""tests/superpoint_train_cases.py against the library and torch on the CPU: the restated layouts equal the library's sizes, the float64
reference equals torch autograd, the tie rule is torch's, every named case has the launch properties it was chosen for, and the integer
cases keep every fp32 sum exact."""
import pytest
import torch
import torch.nn.functional as F

import superpoint_train_cases as cases
from openglue_amd import _lib
from openglue_amd.superpoint import CONV_NAMES, _GRAD_FLOATS, _GRAD_SLICES

SHAPES = [(1, 8, 8), (1, 9, 15), (2, 44, 60), (1, 72, 136), (3, 43, 61), (1, 13, 250), (5, 31, 17), (1, 480, 640)] + \
    [c[:3] for c in cases.CASES.values()]


def test_layouts():
    lib = _lib.load()
    for B, H, W in SHAPES:
        lay = cases.saved_layout(B, H, W)
        assert lay.total * 4 == lib.og_superpoint_train_saved_bytes(B, H, W), (B, H, W)
        spans = sorted((o, o + s[0] * s[1] * s[2] * s[3]) for o, s in lay.fields.values())
        assert spans[0][0] == 0 and all(a[1] <= b[0] < a[1] + 64 and b[0] % 64 == 0 for a, b in zip(spans, spans[1:]))
        assert list(lay.fields)[:2] == ["hidden", "a1a"] and lay.fields["a1a"][0] == cases._round64(B * (H // 8) * (W // 8) * 512)
        # the backward's workspace holds at least the two ping-pong gradient buffers
        assert lib.og_superpoint_train_workspace_bytes(B, H, W, 0) >= 4 * (B * H * W * 64 + B * (H // 2) * (W // 2) * 64)
    # the flat gradient buffer equals the Python side's view of it
    lay, total = cases.grad_layout()
    assert total == _GRAD_FLOATS
    for key, name in [("conv1a", "conv1a")] + [(j, CONV_NAMES[j + 1]) for j in range(7)]:
        assert lay[key] == _GRAD_SLICES[name], name
    (ow, sw), (ob, sb) = lay[7]
    assert _GRAD_SLICES["convPa"] == ((ow, (256, 128, 3, 3)), (ob, (256,)))
    assert _GRAD_SLICES["convDa"] == ((ow + 256 * 128 * 9, (256, 128, 3, 3)), (ob + 256, (256,)))
    assert sw == (512, 128, 3, 3) and sb == (512,)


def _forward64(sd, img):
    """the trunk in float64 with every pre-ReLU tensor kept for autograd: saved fields (NHWC), hidden, the pre-ReLU tensors z[key]"""
    conv = lambda x, name: F.conv2d(x, sd[f"{name}.weight"], sd[f"{name}.bias"], padding=1)
    z, fields = {}, {}
    z["conv1a"] = conv(img, "conv1a")
    x = F.relu(z["conv1a"])
    fields["a1a"] = x
    for j, name in enumerate(cases.LAYER_NAMES[:7]):
        z[j] = conv(x, name)
        x = F.relu(z[j])
        if cases.POOLED[j]:
            fields[f"pre{j}"] = x
            x = F.max_pool2d(x, 2)
        fields[f"act{j}"] = x
    z[7] = torch.cat([conv(x, "convPa"), conv(x, "convDa")], 1)
    for t in z.values():
        t.retain_grad()
    return {k: cases.nhwc(v).detach() for k, v in fields.items()}, F.relu(z[7]), z


@pytest.mark.parametrize("first_layer", [0, 3, 8])
def test_reference_equals_autograd(first_layer):
    """26 x 22: the second pool drops a row and a column (13 x 11 -> 6 x 5), the third a column (6 x 5 -> 3 x 2)"""
    gen = torch.Generator().manual_seed(11)
    B, H, W = 2, 26, 22
    names = ["conv1a"] + cases.LAYER_NAMES[:7] + ["convPa", "convDa"]
    shapes = [(64, 1)] + [(co, ci) for ci, co in cases.LAYERS[:7]] + [(256, 128), (256, 128)]
    sd = {}
    for name, (co, ci) in zip(names, shapes):
        sd[f"{name}.weight"] = (torch.randn(co, ci, 3, 3, generator=gen, dtype=torch.float64) * (2 / (9 * ci)) ** 0.5).requires_grad_(True)
        sd[f"{name}.bias"] = (0.1 * torch.randn(co, generator=gen, dtype=torch.float64)).requires_grad_(True)
    img = torch.randn(B, 1, H, W, generator=gen, dtype=torch.float64)
    fields, hidden, z = _forward64(sd, img)
    G = torch.randn(hidden.shape, generator=gen, dtype=torch.float64)
    (hidden * G).sum().backward()
    weights = {j: sd[f"{n}.weight"].detach() for j, n in enumerate(cases.LAYER_NAMES[:7])}
    weights[7] = torch.cat([sd["convPa.weight"], sd["convDa.weight"]]).detach()
    g_hidden = cases.nhwc(G * (hidden.detach() > 0))
    ref = cases.backward_reference({k: fields[k] for k in cases.fields_needed(first_layer)}, g_hidden, weights, img, first_layer, torch.float64)

    run = cases.layers_run(first_layer)
    assert set(ref) == set(run) | {"worst_cond"} | ({"conv1a"} if first_layer == 0 else set())
    assert run == list(range(7, max(first_layer - 1, 0) - 1, -1))
    close = lambda a, b: float((a - b).abs().max()) <= 1e-12 * float(b.abs().max())
    for key in [k for k in ref if k != "worst_cond"]:
        if key == 7:
            dW = torch.cat([sd["convPa.weight"].grad, sd["convDa.weight"].grad])
            db = torch.cat([sd["convPa.bias"].grad, sd["convDa.bias"].grad])
        else:
            name = "conv1a" if key == "conv1a" else cases.LAYER_NAMES[key]
            dW, db = sd[f"{name}.weight"].grad, sd[f"{name}.bias"].grad
        assert close(ref[key]["dW"], dW) and close(ref[key]["db"], db), key
        assert close(ref[key]["dump"], z[key].grad), key
        assert bool((ref[key]["cond_dW"] >= ref[key]["dW"].abs()).all()) and bool((ref[key]["cond_dump"] >= ref[key]["dump"].abs()).all())
    # the pool did drop pixels, and they carry exactly 0
    d2 = ref[2]["dump"] if 2 in ref else None
    if d2 is not None:
        assert d2.shape[2:] == (13, 11) and float(d2[:, :, 12].abs().max()) == 0.0 and float(d2[:, :, :, 10].abs().max()) == 0.0
        assert float(d2.abs().max()) > 0.0


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("channels_last", [False, True])
def test_tie_rule_is_torch(dtype, channels_last):
    """windows full of equal positive values: torch's max_pool2d backward picks the first maximum in raster order, and so does route"""
    gen = torch.Generator().manual_seed(5)
    pre = torch.randint(0, 3, (2, 8, 9, 11), generator=gen).to(dtype)
    assert int((pre.unfold(2, 2, 2).unfold(3, 2, 2).flatten(-2).max(-1, keepdim=True).values ==
                pre.unfold(2, 2, 2).unfold(3, 2, 2).flatten(-2)).sum(-1).max()) == 4          # a window with a four-way tie
    if channels_last:
        pre = pre.contiguous(memory_format=torch.channels_last)
    pre.requires_grad_(True)
    g = torch.randint(1, 5, (2, 8, 4, 5), generator=gen).to(dtype)
    F.max_pool2d(pre, 2).backward(g)
    mine = cases.route(g, pre.detach())
    assert torch.equal(mine, pre.grad)
    assert float(mine[:, :, 8].abs().max()) == 0.0 and float(mine[:, :, :, 10].abs().max()) == 0.0
    # hand-made: maximum at positions 1 and 2 -> position 1 (upper right) takes it
    pre = torch.tensor([[1.0, 2.0], [2.0, 0.0]], dtype=dtype).view(1, 1, 2, 2)
    assert cases.route(torch.full((1, 1, 1, 1), 7.0, dtype=dtype), pre).flatten().tolist() == [0.0, 7.0, 0.0, 0.0]


def _splits(B, H, W, j):
    h, w = cases.layer_dims(j, H, W)
    per, S = cases.wgrad_split(B, h, w, *cases.LAYERS[j])
    total = cases.tiles(B, h, w)
    return per, S, total, total - (S - 1) * per, total // B


def test_case_properties():
    """each named case has the launch properties it was chosen for; a changed constant in the source shows up here"""
    assert cases.constants() == (512, 512, 1024)
    # wide: all layers, multi-tile splits, short last splits, splits that cross images, partial tile columns, dropped columns
    B, H, W, first = cases.CASES["wide"]
    sp = [_splits(B, H, W, j) for j in range(8)]
    assert first == 0 and [s[0] for s in sp] == [5, 2, 2, 1, 2, 1, 1, 4]
    assert sp[0][3] == 1 and sp[7][3] == 3 and sp[7][0] == 4                         # last split: 1 tile of 5 at conv1b, 3 of 4 at the heads
    for j in (0, 7):                                                                 # a split that holds tiles of two images (207 tiles per image in fives, 9 in fours)
        per, S, total, last, per_image = sp[j]
        assert any((s * per) // per_image != (min(total, (s + 1) * per) - 1) // per_image for s in range(S)), j
    assert [cases.layer_dims(j, H, W) for j in (0, 1, 3, 5)] == [(24, 1100), (12, 550), (6, 275), (3, 137)]
    assert 1100 % 16 and 550 % 16 and 275 % 16 and 137 % 16 and 275 % 2 and 137 % 2 and (24 + 7) // 8 == 3
    assert -(-B * H * W // 1024) == 78 and B * H * W - 77 * 1024 == 352
    assert all(cases.dgrad_form(j, cases.tiles(B, *cases.layer_dims(j, H, W)))[0] == 64 for j in range(8))
    # many: the 128-channel data gradients, unpooled at layers 7, 6, 5 and pooled at layer 4
    B, H, W, first = cases.CASES["many"]
    assert first == 4 and cases.layers_run(first) == [7, 6, 5, 4, 3]
    assert cases.tiles(B, 2, 17) == 514 and cases.tiles(B, 4, 34) == 771
    assert [cases.dgrad_form(j, cases.tiles(B, *cases.layer_dims(j, H, W))) for j in (7, 6, 5, 4)] == \
        [(128, False), (128, False), (128, False), (128, True)]
    sp = [_splits(B, H, W, j) for j in (7, 6, 5, 4, 3)]
    assert [s[0] for s in sp] == [65, 17, 17, 25, 13] and [s[3] for s in sp] == [59, 4, 4, 21, 4]
    assert all(s[0] > 2 * s[4] for s in sp)                                          # every full split spans several images
    # edge: the other side of the threshold at the same layers
    B, H, W, first = cases.CASES["edge"]
    assert first == 5 and cases.tiles(B, 2, 17) == 510
    assert [cases.dgrad_form(j, 510) for j in (7, 6, 5)] == [(64, False)] * 3
    assert cases.dgrad_form(7, 511)[0] == 64 and cases.dgrad_form(7, 512)[0] == 128 and cases.dgrad_form(3, 10 ** 6)[0] == 64
    # small: one tile per split everywhere
    B, H, W, first = cases.CASES["small"]
    assert first == 0 and all(_splits(B, H, W, j)[0] == 1 for j in range(8))
    # the predicted launch lists name all four data-gradient instances
    names = {n for c in cases.CASES.values() for n in cases.launch_list(*c)}
    assert {f"sp_dgrad_kernel<SpPlain, {bn}, {p}>" for bn in (64, 128) for p in ("true", "false")} <= names
    assert cases.launch_list(1, 8, 8, 8) == ["sp_wgrad_kernel<SpPlain, false, false>", "sp_reduce_parts_kernel", "sp_reduce_parts_kernel", "sp_grad_dump_kernel<SpPlain, false>"]


@pytest.mark.parametrize("case", list(cases.CASES))
def test_integer_case_is_exact(case):
    B, H, W, first = cases.CASES[case]
    data = cases.integer_case(B, H, W, first, seed=1)
    assert set(data["fields"]) == set(cases.fields_needed(first))
    for j, (ci, co) in enumerate(cases.LAYERS):
        w = data["weights"][j]
        assert w.shape == (co, ci, 3, 3) and bool(((w != 0).sum((0, 2, 3)) == 8).all()) and set(w.unique().tolist()) == {-1.0, 0.0, 1.0}
    for j in (0, 2, 4):
        if f"pre{j}" in data["fields"] and f"act{j}" in data["fields"]:
            pre, act = data["fields"][f"pre{j}"], data["fields"][f"act{j}"]
            assert torch.equal(cases.nhwc(F.max_pool2d(cases.nchw(pre, torch.float32), 2)), act)
            win = cases.nchw(pre, torch.float32)[:, :, :pre.shape[1] // 2 * 2, :pre.shape[2] // 2 * 2].unfold(2, 2, 2).unfold(3, 2, 2).flatten(-2)
            ties = ((win == win.max(-1, keepdim=True).values).sum(-1) > 1) & (win.max(-1).values > 0)
            assert float(ties.float().mean()) > 0.25, j                              # ties between positive values are abundant
    ref = cases.backward_reference(data["fields"], data["g_hidden"], data["weights"], data["image"], first, torch.float64, exact=True)
    print(f"{case}: worst condition number {ref['worst_cond']:.3e} ({2 ** 24 / ref['worst_cond']:.1f}x below 2^24)")
    assert ref["worst_cond"] < 2 ** 24
    for key in [k for k in ref if k != "worst_cond"]:
        assert bool((ref[key]["dW"] == ref[key]["dW"].round()).all())
        assert float((ref[key]["dW"] != 0).float().mean()) > 0.9, key                # the weight gradient is dense
