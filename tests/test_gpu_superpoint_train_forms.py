"""The SuperPoint fine-tuning kernels (csrc/superpoint_train.hip) per instance: og_superpoint_train_backward called directly on test-built
saved buffers (tests/superpoint_train_cases.py), every layer read back through the layer_grads dump and judged on its own against a
float64 reference on the CPU, and the launched instances asserted by name (openglue_amd.kernel_trace).

Cases (B, H, W, first_layer; tests/test_superpoint_train_cases_cpu.py asserts what each was chosen for):
    wide   3 x 24 x 1100, 0    all layers; weight-gradient workgroups walk 5, 2, 2, 1, 2, 1, 1, 4 tiles, short last splits, splits that cross
                               images, partial tile columns, two pools that drop a column, sp_wgrad1a_kernel with 78 splits
    many   257 x 16 x 136, 4   514 / 771 tiles: sp_dgrad_kernel<128, false> at the heads, conv4b, conv4a and <128, true> at conv3b; splits of
                               65, 17, 17, 25, 13 tiles, each over several images
    edge   255 x 16 x 136, 5   510 tiles: the other side of the threshold, sp_dgrad_kernel<64, false> at the same layers
    small  2 x 44 x 60, 0      one tile per split, the shape of tests/test_gpu_superpoint_train.py, as the control

test_integer_exact: integer data whose every fp32 sum is exact in any order -> dW, db and every dump equal float64 bit for bit.
test_real_valued_per_layer: normal data; the reference of layer j starts from the GPU's own dump of layer j (checked one step earlier; the
reference applies its own mask and pool routing), so each kernel is judged alone.  Two bars: elementwise |gpu - ref64| <= 2 n 2^-24 cond
(n products per sum, cond the sum of their absolute values), and per tensor err = max|gpu - ref64| / max|ref64| <= FACTOR x the same
figure of ATen fp32 on the CPU (conv2d_input / conv2d_weight, same inputs).  conv1a has no dump: it is judged together with conv1b's
data gradient (both bars through the two steps).
test_saved_activations: og_superpoint_train_forward; the saved planes of sp_conv3x3_save_kernel<64 / 128> and of the layers around them.
test_describe_backward_direct: og_superpoint_describe_backward with more than 64 keypoints on one cell and taps outside the map.

Measured on an MI355X (profiles/superpoint_train_forms_gpu_tests.log; DESIGN.md 4.8b has the table).  Ratio of err to the ATen-fp32 err,
range over the layers of a case, and the worst |gpu - ref64| as a fraction of the hard bound:
    case    dW            db            data gradient (dump of the layer below)                hard bound, worst
    wide    0.16 .. 0.88  1.00 .. 1.96  1.24 .. 1.65  (<64, false>, <64, true>)                 3.1e-3
    many    0.50 .. 0.90  1.08 .. 2.52  1.19 .. 1.55  (<128, false> x 3, <128, true>)           8.4e-4
    small   0.42 .. 0.94  0.71 .. 1.88  1.23 .. 2.11  (<64, false>, <64, true>)                 1.8e-2 (coarse dW, n = 70)
    saved activations (forward)   0.61 .. 3.40 (hidden at 72 x 136)        describe backward 0.68 (a cell of 90 keypoints: 2.1e-7)
Every factor is the project's 4 (FACTOR of tests/test_gpu_superpoint_train.py), the per-layer bias sums included: their worst is 2.52.
What this file found: with one fp32 chain over all 9 x Cout products the data gradient measured 2.2 .. 7.9 x ATen (7.03 / 7.68 / 7.91 at
the heads, K = 4608, in small / wide / many; 4.3 .. 5.0 at K = 1152), inside the hard bound but outside the bar, and hidden by the
whole-network test, where the error of the sums over pixels dominates.  sp_dgrad_kernel now sums every pass of 32 channels x 9 taps on
its own (sp_conv3x3_accumulate<BN, true>) and the figures above are with that.
Breakages tried on a scratch copy of the kernel: a weight-gradient workgroup that skips the last tile of a full split fails
test_integer_exact[wide, many, edge] and test_real_valued_per_layer[wide, many] (small, one tile per split, passes: it is the control);
routing the pool gradient to the last instead of the first maximum fails test_integer_exact for all four cases and nothing else -- real
data never ties.
"""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

import superpoint_train_cases as cases
from openglue_amd import _lib, synthetic as syn
from openglue_amd.kernel_trace import launched_kernels, superpoint_train_instances
from openglue_amd.superpoint import SuperPointNet
from test_gpu_superpoint_train import FACTOR, _describe, _dev, _images, _net

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
GUARD = 1024            # floats = 4 KiB behind the saved buffer; the same number of bytes x 4 behind the workspace
NAN = float("nan")


def _bits(t):
    """fp32 bit pattern, with -0 folded onto +0 (a masked product of the reference may be -0 where the kernel stores +0)"""
    return (t.to(torch.float32) + 0.0).contiguous().view(torch.int32)


def _same(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


@functools.lru_cache(maxsize=None)
def _run(case, kind):
    """One og_superpoint_train_backward of a case on test-built buffers, run twice (the second time under the kernel trace); shared, and
    left unchanged, by the tests that need it."""
    B, H, W, first = cases.CASES[case]
    data = (cases.integer_case if kind == "integer" else cases.real_case)(B, H, W, first, seed=1)
    dev, lib = _dev(), _lib.load()
    lay = cases.saved_layout(B, H, W)
    assert lay.total * 4 == lib.og_superpoint_train_saved_bytes(B, H, W)
    saved = torch.full((lay.total + GUARD,), NAN, device=dev)                        # fields the case does not need stay NaN: nothing may read them
    saved[lay.total:] = 1234.5
    for name, t in data["fields"].items():
        off, shape = lay.fields[name]
        assert tuple(t.shape) == shape
        saved[off:off + t.numel()] = t.reshape(-1).to(dev)
    nws = lib.og_superpoint_train_workspace_bytes(B, H, W, 0)
    assert nws > 0
    ws = torch.full((nws + 4 * GUARD,), 0xA5, dtype=torch.uint8, device=dev)
    glay, gtotal = cases.grad_layout()
    dlay, dtotal = cases.dump_layout(B, H, W)
    grads = torch.full((gtotal,), NAN, device=dev)
    dump = torch.full((dtotal,), NAN, device=dev)
    net = SuperPointNet()
    net.load_state_dict(cases.module_state(data["weights"]))
    pg = net._pack_grad(dev)
    img, gh = data["image"].to(dev).contiguous(), data["g_hidden"].to(dev).contiguous()
    assert ws.data_ptr() % 16 == 0 and saved.data_ptr() % 16 == 0

    def launch():
        _lib.call("og_superpoint_train_backward", dev, B, H, W, img.data_ptr(), pg.data_ptr(), saved.data_ptr(), gh.data_ptr(), first,
                  grads.data_ptr(), dump.data_ptr(), ws.data_ptr(), _lib.STREAM)

    launch()
    torch.cuda.synchronize()
    first_grads = grads.clone()
    names = superpoint_train_instances(launched_kernels(launch))
    run = cases.layers_run(first)
    out = dict(data=data, names=names, grads=grads.cpu(), run=run, first=first, shape=(B, H, W),
               repeat_same=torch.equal(_bits(first_grads), _bits(grads)),
               saved_guard=bool((saved[lay.total:] == 1234.5).all()), ws_guard=bool((ws[nws:] == 0xA5).all()),
               dump={j: dump[dlay[j][0]:dlay[j][0] + math.prod(dlay[j][1])].view(dlay[j][1]).cpu() for j in run},
               dump_unwritten=all(bool(dump[dlay[j][0]:dlay[j][0] + math.prod(dlay[j][1])].isnan().all()) for j in range(8) if j not in run))
    return out


def _grad(r, key):
    (ow, sw), (ob, sb) = cases.grad_layout()[0][key]
    return r["grads"][ow:ow + math.prod(sw)].view(sw), r["grads"][ob:ob + sb[0]]


@pytest.mark.parametrize("case", list(cases.CASES))
def test_integer_exact(case):
    r = _run(case, "integer")
    d, first = r["data"], r["first"]
    ref = cases.backward_reference(d["fields"], d["g_hidden"], d["weights"], d["image"], first, torch.float64, exact=True)
    keys = r["run"] + (["conv1a"] if first == 0 else [])
    assert set(keys) | {"worst_cond"} == set(ref)
    bad = []
    for key in keys:
        dW, db = _grad(r, key)
        assert not dW.isnan().any() and not db.isnan().any(), key
        if not _same(dW, ref[key]["dW"]):
            bad.append((key, "dW", int((dW.double() != ref[key]["dW"]).sum())))
        if not _same(db, ref[key]["db"]):
            bad.append((key, "db", int((db.double() != ref[key]["db"]).sum())))
        if key != "conv1a":
            got = r["dump"][key]
            assert not got.isnan().any(), key
            if not _same(got, cases.nhwc(ref[key]["dump"])):
                bad.append((key, "dump", int((got.double() != cases.nhwc(ref[key]["dump"])).sum())))
    assert not bad, f"{case}: (layer, tensor, elements that differ from float64) {bad}"
    assert _same(r["dump"][7], d["g_hidden"])
    for key in ["conv1a"] + list(range(8)):                                          # layers that do not run: still NaN
        if key not in keys:
            dW, db = _grad(r, key)
            assert bool(dW.isnan().all()) and bool(db.isnan().all()), key
    assert r["dump_unwritten"]
    assert r["saved_guard"] and r["ws_guard"] and r["repeat_same"]


def _judge(tag, cls, gpu, ref64, ref32, cond, n, bad, worst):
    """prints the figures of one tensor, then records a miss of the hard bound or of the tight bar"""
    diff = (gpu.double() - ref64).abs()
    bound = 2.0 * n * U * cond
    hard = float((diff / bound.clamp_min(1e-300)).max()) if bool((diff <= bound).all()) else float("inf")
    den = float(ref64.abs().max())
    e_gpu, e_aten = float(diff.max()) / den, float((ref32.double() - ref64).abs().max()) / den
    ratio = e_gpu / max(e_aten, 1e-30)
    print(f"{tag:24s} max|ref| {den:.3e}  gpu {e_gpu:.2e}  aten-fp32 {e_aten:.2e}  ratio {ratio:.2f} (bar {FACTOR:g})  worst |diff| / hard bound {hard:.2e} (n = {n})")
    worst[cls] = max(worst.get(cls, 0.0), ratio)
    if not hard <= 1.0:
        bad.append((tag, "hard bound"))
    if not e_gpu <= FACTOR * e_aten:
        bad.append((tag, f"ratio {ratio:.2f}"))


@pytest.mark.parametrize("case", ["wide", "many", "small"])
def test_real_valued_per_layer(case):
    r = _run(case, "real")
    d, first, (B, H, W) = r["data"], r["first"], r["shape"]
    f = d["fields"]
    bad, worst = [], {}
    assert _same(r["dump"][7], d["g_hidden"])
    for j in r["run"]:
        h, w = cases.layer_dims(j, H, W)
        cout = cases.LAYERS[j][1]
        xname = "a1a" if j == 0 else f"act{j - 1}"
        g32 = cases.nchw(r["dump"][j], torch.float32)                                # the GPU's own full-resolution gradient of this layer
        assert not g32.isnan().any(), j
        s64 = cases.layer_step(g32.double(), cases.nchw(f[xname], torch.float64), d["weights"][j].double(), need_dx=j >= first)
        s32 = cases.layer_step(g32, cases.nchw(f[xname], torch.float32), d["weights"][j], need_dx=j >= first, cond=False)
        dW, db = _grad(r, j)
        name = cases.LAYER_NAMES[j]
        _judge(f"{case} {name} dW", "dW", dW, s64["dW"], s32["dW"], s64["cond_dW"], B * h * w, bad, worst)
        _judge(f"{case} {name} db", "db", db, s64["db"], s32["db"], s64["cond_db"], B * h * w, bad, worst)
        if j < first:
            continue
        dx64, dx32, cdx = s64["dx"], s32["dx"], s64["cond_dx"]
        if j == 0:                                                                   # conv1a: through conv1b's data gradient, no dump in between
            img = d["image"]
            c64, c32 = cases.conv1a_step(dx64, img.double(), cond_g=cdx), cases.conv1a_step(dx32, img)
            dW, db = _grad(r, "conv1a")
            n = 9 * cout + B * H * W
            _judge(f"{case} conv1a dW (+dgrad)", "dW", dW, c64["dW"], c32["dW"], c64["cond_dW"], n, bad, worst)
            _judge(f"{case} conv1a db (+dgrad)", "db", db, c64["db"], c32["db"], c64["cond_db"], n, bad, worst)
            continue
        if cases.POOLED[j - 1]:
            pre = cases.nchw(f[f"pre{j - 1}"], torch.float64)
            dx64, dx32, cdx = cases.route(dx64, pre), cases.route(dx32, pre.float()), cases.route(cdx, pre)
        got = cases.nchw(r["dump"][j - 1], torch.float32)
        bn, pooled = cases.dgrad_form(j, cases.tiles(B, h, w))
        _judge(f"{case} {name} dgrad<{bn},{int(pooled)}>", "dgrad", got, dx64, dx32, cdx, 9 * cout, bad, worst)
    print(f"{case}: worst ratio per class {', '.join(f'{k} {v:.2f}' for k, v in sorted(worst.items()))}")
    assert not bad, f"{case}: {bad}"
    assert r["saved_guard"] and r["ws_guard"] and r["repeat_same"]


def test_instances():
    """the launches of every case, in order, are those the restated launcher arithmetic predicts; over the module every data-gradient,
    weight-gradient and dump instance has run"""
    seen = set()
    norm = lambda names: [n.replace(" ", "") for n in names]
    for case, c in cases.CASES.items():
        print(case, _run(case, "integer")["names"])
        got = norm(_run(case, "integer")["names"])
        assert got == norm(cases.launch_list(*c)), case
        seen |= set(got)
    layers = lambda case: [n for n in norm(_run(case, "integer")["names"]) if n.startswith("sp_dgrad_kernel<SpPlain,")]
    assert layers("edge") == ["sp_dgrad_kernel<SpPlain,64,false>"] * 3 and layers("many")[:3] == ["sp_dgrad_kernel<SpPlain,128,false>"] * 3
    assert layers("many")[3] == "sp_dgrad_kernel<SpPlain,128,true>"
    want = {f"sp_dgrad_kernel<SpPlain,{bn},{p}>" for bn in (64, 128) for p in ("true", "false")} | \
        {f"sp_wgrad_kernel<SpPlain,{p},false>" for p in ("true", "false")} | {f"sp_grad_dump_kernel<SpPlain,{p}>" for p in ("true", "false")} | \
        {"sp_wgrad1a_kernel<SpPlain>", "sp_reduce_parts_kernel"}
    assert want <= seen, want - seen


@pytest.mark.parametrize("shape", [(2, 44, 60), (1, 72, 136)], ids=["b2_44x60", "b1_72x136"])
def test_saved_activations(shape):
    B, H, W = shape
    dev, lib = _dev(), _lib.load()
    net = _net()
    img = _images(B, H, W)
    lay = cases.saved_layout(B, H, W)
    saved = torch.full((lay.total + GUARD,), NAN, device=dev)
    saved[lay.total:] = 1234.5
    heat = torch.empty(B, H // 8 * 8, W // 8 * 8, device=dev)
    desc = torch.empty(B, H // 8, W // 8, 256, device=dev)
    packed, gimg = net._pack(dev), img.to(dev).contiguous()
    names = superpoint_train_instances(launched_kernels(lambda: _lib.call(
        "og_superpoint_train_forward", dev, B, H, W, gimg.data_ptr(), packed.data_ptr(), saved.data_ptr(), heat.data_ptr(), desc.data_ptr(), _lib.STREAM)))
    assert [n.replace(" ", "") for n in names] == ["sp_conv3x3_save_kernel<64>", "sp_conv3x3_save_kernel<64>", "sp_conv3x3_save_kernel<128>"]
    assert bool((saved[lay.total:] == 1234.5).all())
    saved = saved.cpu()
    field = lambda name: saved[lay.fields[name][0]:lay.fields[name][0] + math.prod(lay.fields[name][1])].view(lay.fields[name][1])
    for name in lay.fields:
        assert not field(name).isnan().any(), name                                   # every plane fully written
    sd = syn.make_superpoint_state_dict(False, seed=1)
    bad, worst = [], {}

    def judge(tag, got, x, wname):
        """got [B, h, w, C] against relu(conv(x) + b) of the GPU's own saved input x, float64 and ATen fp32"""
        w, b = (torch.cat([sd[f"{n}.{k}"] for n in wname]) for k in ("weight", "bias"))
        ref = lambda dt: F.relu(F.conv2d(x.to(dt), w.to(dt), b.to(dt), padding=1))
        r64, r32 = ref(torch.float64), ref(torch.float32)
        den = float(r64.abs().max())
        e_gpu, e_aten = float((cases.nchw(got, torch.float64) - r64).abs().max()) / den, float((r32.double() - r64).abs().max()) / den
        print(f"{B}x{H}x{W} {tag:16s} max|ref| {den:.3e}  gpu {e_gpu:.2e}  aten-fp32 {e_aten:.2e}  ratio {e_gpu / max(e_aten, 1e-30):.2f}")
        worst[tag] = e_gpu / max(e_aten, 1e-30)
        if not e_gpu <= FACTOR * e_aten:
            bad.append((tag, e_gpu, e_aten))

    judge("a1a", field("a1a"), img, ["conv1a"])
    for j, name in enumerate(cases.LAYER_NAMES[:7]):
        x = cases.nchw(field("a1a" if j == 0 else f"act{j - 1}"), torch.float32)
        if cases.POOLED[j]:
            pre, act = field(f"pre{j}"), field(f"act{j}")
            assert torch.equal(_bits(cases.nhwc(F.max_pool2d(cases.nchw(pre, torch.float32), 2))), _bits(act)), name
            judge(f"pre{j} {name}", pre, x, [name])
        else:
            judge(f"act{j} {name}", field(f"act{j}"), x, [name])
    judge("hidden", field("hidden"), cases.nchw(field("act6"), torch.float32), ["convPa", "convDa"])
    assert not bad, f"saved activations above {FACTOR} x ATen-fp32: {bad}"


def _describe_case():
    """B = 2, Hc x Wc = 3 x 5 (24 x 40 pixels), n = 130 keypoints (y, x) per image.  Image 0: the four corners, all 64 pixels of the
    interior cell (1, 2), pixels of the outer 4-pixel ring on each side, and 26 pixels right of the cell that sample the same coarse
    cell; image 1: 130 distinct seeded pixels."""
    gen = torch.Generator().manual_seed(7)
    pick = lambda pts, k: [pts[i] for i in torch.randperm(len(pts), generator=gen)[:k].tolist()]
    pts = [(0, 0), (0, 39), (23, 0), (23, 39)]
    pts += [(y, x) for y in range(8, 16) for x in range(16, 24)]
    pts += pick([(y, x) for y in range(0, 4) for x in range(4, 36)], 10) + pick([(y, x) for y in range(20, 24) for x in range(4, 36)], 10)
    pts += pick([(y, x) for y in range(4, 7) for x in range(0, 4)], 8) + pick([(y, x) for y in range(14, 20) for x in range(36, 40)], 8)
    pts += [(y, x) for y in range(8, 15) for x in range(24, 28)][:26]
    assert len(pts) == 130 and len(set(pts)) == 130
    idx0 = torch.tensor([y * 40 + x for y, x in pts])
    idx1 = torch.randperm(24 * 40, generator=gen)[:130]
    idx = torch.stack([idx0, idx1])
    coarse = F.normalize(torch.randn(2, 3, 5, 256, generator=gen), dim=-1)
    dd = torch.randn(2, 130, 256, generator=gen)
    return idx, coarse, dd


def test_describe_backward_direct():
    B, Hc, Wc, n, ld = 2, 3, 5, 130, 136
    idx, coarse, dd = _describe_case()
    xy = torch.stack([idx % (Wc * 8), idx // (Wc * 8)], -1).double()                 # [B, n, (x, y)]
    # which cells each keypoint touches, in float64 (no pixel lies within 1e-3 of a cell boundary of the sampling grid, four thousand fp32 ulps)
    ix = ((xy[..., 0] - 3.5) / (Wc * 8 - 4.5) * 2 * Wc - 1) / 2
    iy = ((xy[..., 1] - 3.5) / (Hc * 8 - 4.5) * 2 * Hc - 1) / 2
    assert float(torch.minimum((ix - ix.round()).abs().min(), (iy - iy.round()).abs().min())) > 1e-3
    x0, y0 = ix.floor().long(), iy.floor().long()
    assert int(x0[0].min()) == -1 and int(y0[0].min()) <= -1 and int(x0[0].max()) == Wc - 1 and int(y0[0].max()) == Hc - 1
    count = torch.zeros(B, Hc, Wc, dtype=torch.long)
    hits = [[], []]
    for b in range(B):
        for k in range(n):
            for cy in (int(y0[b, k]), int(y0[b, k]) + 1):
                for cx in (int(x0[b, k]), int(x0[b, k]) + 1):
                    if 0 <= cy < Hc and 0 <= cx < Wc:
                        count[b, cy, cx] += 1
                        if (b, cy, cx) == (0, 1, 2):
                            hits[0].append(k)
    assert int(count[0, 1, 2]) > 64 and len({k // 64 for k in hits[0]}) >= 2         # one cell gathers over more than one ballot step
    untouched = count == 0
    assert int(untouched[0].sum()) >= 1

    dev = _dev()
    sel = torch.full((B, ld), 2 ** 30, dtype=torch.int32)                            # entries past n are never read
    sel[:, :n] = idx.int()
    sel, gc, gd = sel.to(dev), coarse.to(dev).contiguous(), dd.to(dev).contiguous()
    nws = B * n * (256 + 8) * 4
    ws = torch.full((nws + 4 * GUARD,), 0xA5, dtype=torch.uint8, device=dev)
    out = torch.full((B, Hc, Wc, 256), NAN, device=dev)
    launch = lambda: _lib.call("og_superpoint_describe_backward", dev, B, Hc, Wc, n, sel.data_ptr(), ld, gc.data_ptr(), gd.data_ptr(),
                               out.data_ptr(), ws.data_ptr(), _lib.STREAM)
    launch()
    torch.cuda.synchronize()
    got = out.cpu()
    out.fill_(NAN)
    names = superpoint_train_instances(launched_kernels(launch))
    assert names == ["sp_describe_bwd_point_kernel", "sp_describe_bwd_cell_kernel"]
    assert torch.equal(_bits(got), _bits(out.cpu()))                                 # a second run: the same bits
    assert bool((ws[nws:] == 0xA5).all())
    assert not got.isnan().any()                                                     # d_coarse fully overwritten

    def oracle(dtype):
        cd = coarse.to(dtype).requires_grad_(True)
        sum((_describe(cd[b], xy[b], dtype) * dd[b].to(dtype)).sum() for b in range(B)).backward()
        return cd.grad

    g64, g32 = oracle(torch.float64), oracle(torch.float32)
    assert float(g64[untouched].abs().max()) == 0.0
    assert float(got[untouched].abs().max()) == 0.0                                  # cells no keypoint touches: exactly 0
    den = float(g64.abs().max())
    e_gpu, e_aten = float((got.double() - g64).abs().max()) / den, float((g32.double() - g64).abs().max()) / den
    print(f"describe backward: max|g| {den:.3e}  gpu {e_gpu:.2e}  aten-fp32 {e_aten:.2e}  ratio {e_gpu / max(e_aten, 1e-30):.2f}")
    for b in range(B):
        for cy in range(Hc):
            for cx in range(Wc):
                if count[b, cy, cx] > 64:
                    e = float((got[b, cy, cx].double() - g64[b, cy, cx]).abs().max()) / den
                    print(f"  cell ({b}, {cy}, {cx}) with {int(count[b, cy, cx])} keypoints: gpu {e:.2e}")
    assert e_gpu <= FACTOR * e_aten
