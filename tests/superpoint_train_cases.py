"""Cases and float64 references for the per-kernel tests of csrc/superpoint_train.hip and the bodies it takes from csrc/og_superpoint_train.h (tests/test_superpoint_train_cases_cpu.py checks this
file against the library and torch autograd on the CPU; tests/test_gpu_superpoint_train_forms.py runs the kernels against it).

Everything here is plain torch on the CPU.  The launcher's arithmetic is restated (saved_layout, wgrad_split, dgrad_form, launch_list);
its constants -- SPW_TARGET_WGS, the `tiles < 512` rule of the data gradient, SP_1A_PIX -- are read out of the shared header, so that a
changed constant fails test_case_properties instead of silently moving a case off the launch form it was chosen for.

Layers are the eight MFMA layers j = 0..7 of the source (conv1b, 2a, 2b, 3a, 3b, 4a, 4b, heads Pa | Da); conv1a is "conv1a".
`first_layer` is the C argument: an index into conv1a, conv1b, ..., conv4b (8 = heads only), the lowest layer that needs a gradient.
Tensors that mirror device buffers are NHWC float32 ("fields"); the references compute in NCHW in the dtype they are given.
"""
import os
import re
from types import SimpleNamespace

import torch
import torch.nn.functional as F
from torch.nn.grad import conv2d_input, conv2d_weight

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "openglue_amd", "csrc", "og_superpoint_train.h")       # the launcher both SuperPoint training units share
LAYERS = [(64, 64), (64, 64), (64, 64), (64, 128), (128, 128), (128, 128), (128, 128), (128, 512)]       # (Cin, Cout)
POOLED = (True, False, True, False, True, False, False, False)
SHIFT = (0, 1, 1, 2, 2, 3, 3, 3)                     # layer j convolves at (H >> SHIFT[j], W >> SHIFT[j])
LAYER_NAMES = ["conv1b", "conv2a", "conv2b", "conv3a", "conv3b", "conv4a", "conv4b", "heads"]
TILE_H, TILE_W = 8, 16                               # SP_TH, SP_TW of og_superpoint_dense.h

# name -> (B, H, W, first_layer); what each was chosen for is asserted by test_case_properties
CASES = {
    "wide": (3, 24, 1100, 0),
    "many": (257, 16, 136, 4),
    "edge": (255, 16, 136, 5),
    "small": (2, 44, 60, 0),
}


# ---------------------------------------------------------------- the launcher's arithmetic
def _constant(pattern):
    found = re.findall(pattern, open(SOURCE).read())
    assert len(found) == 1, f"{SOURCE}: expected exactly one match of {pattern!r}, found {found}"
    return int(found[0])


def constants():
    """(SPW_TARGET_WGS, the tile count from which Cin == 128 layers take sp_dgrad_kernel<128, .>, SP_1A_PIX), read from the source"""
    return (_constant(r"constexpr\s+int\s+SPW_TARGET_WGS\s*=\s*(\d+)\s*;"),
            _constant(r"if\s*\(\s*Cin\s*==\s*64\s*\|\|\s*tiles\s*<\s*(\d+)\s*\)"),
            _constant(r"constexpr\s+int64_t\s+SP_1A_PIX\s*=\s*(\d+)\s*;"))


def layer_dims(j, H, W):
    return H >> SHIFT[j], W >> SHIFT[j]


def tiles(B, h, w):
    return B * ((h + TILE_H - 1) // TILE_H) * ((w + TILE_W - 1) // TILE_W)


def wgrad_split(B, h, w, Cin, Cout):
    """(tiles_per, S) of a sp_wgrad_kernel launch, as Split wgrad_split()"""
    total = tiles(B, h, w)
    blocks = (Cin // 32) * (Cout // 32)
    S = (constants()[0] + blocks - 1) // blocks
    S = 1 if S < 1 else total if S > total else S
    per = (total + S - 1) // S
    return per, (total + per - 1) // per


def dgrad_form(j, ntiles):
    """(BN, POOLED) of the sp_dgrad_kernel instance that layer j takes with `ntiles` pixel tiles"""
    return (64 if LAYERS[j][0] == 64 or ntiles < constants()[1] else 128), POOLED[j]


def layers_run(first_layer):
    """the MFMA layers whose weight gradient runs, top down"""
    return [j for j in range(7, -1, -1) if j + 1 >= first_layer]


def launch_list(B, H, W, first_layer, dump=True):
    """the kernels of one og_superpoint_train_backward call, in launch order, by their short names (SpPlain: SuperPointNet's instances of
    the bodies in og_superpoint_train.h; the third argument of sp_wgrad_kernel, INPOOL, is always false for this network)"""
    b = lambda v: "true" if v else "false"
    out = []
    for j in layers_run(first_layer):
        h, w = layer_dims(j, H, W)
        out += [f"sp_wgrad_kernel<SpPlain, {b(POOLED[j])}, false>", "sp_reduce_parts_kernel", "sp_reduce_parts_kernel"]
        if dump:
            out.append(f"sp_grad_dump_kernel<SpPlain, {b(POOLED[j])}>")
        if j >= first_layer:
            bn, pooled = dgrad_form(j, tiles(B, h, w))
            out.append(f"sp_dgrad_kernel<SpPlain, {bn}, {b(pooled)}>")
    if first_layer == 0:
        out += ["sp_wgrad1a_kernel<SpPlain>", "sp_reduce_parts_kernel", "sp_reduce_parts_kernel"]
    return out


# ---------------------------------------------------------------- buffer layouts
def _round64(n):
    return (n + 63) // 64 * 64


def saved_layout(B, H, W):
    """Saved saved_layout() of the source: .fields name -> (offset in floats, NHWC shape), .total floats.  Names: hidden, a1a, act0..act6
    (the post-ReLU output of layer j, pooled for the pooled layers) and pre0, pre2, pre4 (before the pool)."""
    fields, o = {}, 0

    def take(name, shape):
        nonlocal o
        fields[name] = (o, shape)
        o += _round64(shape[0] * shape[1] * shape[2] * shape[3])

    take("hidden", (B, H // 8, W // 8, 512))
    take("a1a", (B, H, W, 64))
    for j in range(7):
        h, w = layer_dims(j, H, W)
        if POOLED[j]:
            take(f"pre{j}", (B, h, w, LAYERS[j][1]))
            take(f"act{j}", (B, h // 2, w // 2, LAYERS[j][1]))
        else:
            take(f"act{j}", (B, h, w, LAYERS[j][1]))
    return SimpleNamespace(fields=fields, total=o)


def dump_layout(B, H, W):
    """the layer_grads buffer: per layer j (offset in floats, NHWC shape of its full-resolution pre-activation gradient), and the total"""
    out, o = [], 0
    for j in range(8):
        h, w = layer_dims(j, H, W)
        out.append((o, (B, h, w, LAYERS[j][1])))
        o += B * h * w * LAYERS[j][1]
    return out, o


def grad_layout():
    """the flat gradient buffer: key ("conv1a" or j) -> ((offset, shape) of dW, (offset, shape) of db), and the total"""
    out = {"conv1a": ((0, (64, 1, 3, 3)), (576, (64,)))}
    o = 640
    for j, (ci, co) in enumerate(LAYERS):
        out[j] = ((o, (co, ci, 3, 3)), (o + co * ci * 9, (co,)))
        o += co * ci * 9 + co
    return out, o


def fields_needed(first_layer):
    """the saved fields that a backward with this first_layer reads"""
    run = layers_run(first_layer)
    names = ["a1a" if j == 0 else f"act{j - 1}" for j in run]
    return names + [f"pre{j}" for j in run if POOLED[j]]


# ---------------------------------------------------------------- references
def nchw(t, dtype):
    return t.permute(0, 3, 1, 2).to(dtype)


def nhwc(t):
    return t.permute(0, 2, 3, 1)


def route(g_pooled, pre):
    """backward of the 2 x 2 max-pool (NCHW): the pooled gradient goes to the first maximum of each window in raster order; the last
    row / column of an odd size, which no window covers, receive exactly 0"""
    B, C, h, w = pre.shape
    hp, wp = h // 2, w // 2
    win = pre[:, :, :2 * hp, :2 * wp].reshape(B, C, hp, 2, wp, 2).permute(0, 1, 2, 4, 3, 5).reshape(B, C, hp, wp, 4)
    is_max = win == win.max(dim=-1, keepdim=True).values
    first = is_max & (is_max.cumsum(-1) == 1)
    full = (first * g_pooled.unsqueeze(-1)).reshape(B, C, hp, wp, 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(B, C, 2 * hp, 2 * wp)
    return F.pad(full, (0, w - 2 * wp, 0, h - 2 * hp))


def layer_step(dump, x, weight, need_dx, cond=True):
    """One layer of the backward from its full-resolution pre-activation gradient `dump` [B, Cout, h, w], its input x [B, Cin, h, w]
    (post-ReLU, so x >= 0) and its weight [Cout, Cin, 3, 3]: dW, db, and with need_dx the gradient dx of the pre-activation below,
    masked by x > 0.  cond_*: the same sums over the absolute values of their terms."""
    out = {"dW": conv2d_weight(x, weight.shape, dump, padding=1), "db": dump.sum((0, 2, 3))}
    a = dump.abs() if cond else None
    if cond:
        out["cond_dW"] = conv2d_weight(x, weight.shape, a, padding=1)
        out["cond_db"] = a.sum((0, 2, 3))
    if need_dx:
        mask = x > 0
        out["dx"] = conv2d_input(x.shape, weight, dump, padding=1) * mask
        if cond:
            out["cond_dx"] = conv2d_input(x.shape, weight.abs(), a, padding=1) * mask
    return out


def conv1a_step(g, image, cond_g=None):
    """conv1a from the gradient g [B, 64, H, W] of its pre-activation and the image [B, 1, H, W]; cond_g defaults to |g|"""
    a = g.abs() if cond_g is None else cond_g
    return {"dW": conv2d_weight(image, (64, 1, 3, 3), g, padding=1), "db": g.sum((0, 2, 3)),
            "cond_dW": conv2d_weight(image.abs(), (64, 1, 3, 3), a, padding=1), "cond_db": a.sum((0, 2, 3))}


def backward_reference(saved, g_hidden, weights, image, first_layer, dtype, exact=False):
    """The chain of og_superpoint_train_backward in `dtype`.  saved: name -> NHWC field (fields_needed(first_layer) suffice), g_hidden
    [B, Hc, Wc, 512] (already masked by hidden > 0, as the caller of the C entry hands it over), weights[j] [Cout, Cin, 3, 3].
    Returns {j or "conv1a": dW, db, dump (NCHW), cond_dW, cond_db, cond_dump} for exactly the layers the C loop runs, and "worst_cond",
    the largest condition number of the chain.  exact=True asserts worst_cond < 2^24: with integer data every fp32 partial sum, in any
    order, is then an integer below 2^24 in magnitude, hence exact."""
    res = {}
    g = nchw(g_hidden, dtype)
    cg = g.abs()
    worst = float(cg.max())
    for j in layers_run(first_layer):
        x = nchw(saved["a1a" if j == 0 else f"act{j - 1}"], dtype)
        if POOLED[j]:
            pre = nchw(saved[f"pre{j}"], dtype)
            g, cg = route(g, pre), route(cg, pre)
        step = layer_step(g, x, weights[j].to(dtype), need_dx=j >= first_layer)
        res[j] = {"dW": step["dW"], "db": step["db"], "dump": g, "cond_dW": step["cond_dW"], "cond_db": step["cond_db"], "cond_dump": cg}
        worst = max(worst, float(step["cond_dW"].max()), float(step["cond_db"].max()))
        if j < first_layer:
            break
        g, cg = step["dx"], step["cond_dx"]
        worst = max(worst, float(cg.max()))
    if first_layer == 0:
        res["conv1a"] = dict(conv1a_step(g, image.to(dtype)), dump=g, cond_dump=cg)
        worst = max(worst, float(res["conv1a"]["cond_dW"].max()), float(res["conv1a"]["cond_db"].max()))
    res["worst_cond"] = worst
    if exact:
        assert worst < 2 ** 24, f"integer case: condition number {worst:.3e} is not below 2^24, fp32 sums are no longer exact"
    return res


# ---------------------------------------------------------------- data
def _fields(B, H, W, first_layer, draw):
    """the saved fields a case needs; draw(shape) -> a non-negative NHWC field; act = max_pool2d(pre) where the pool's input is needed"""
    need = set(fields_needed(first_layer))
    lay = saved_layout(B, H, W).fields
    out = {}
    for name in sorted(need):
        if name in out:
            continue
        if name.startswith("pre") or not (name.startswith("act") and POOLED[int(name[3:])] and f"pre{name[3:]}" in need):
            out[name] = draw(lay[name][1])
    for name in sorted(need):
        if name not in out:
            out[name] = nhwc(F.max_pool2d(nchw(out[f"pre{name[3:]}"], torch.float32), 2)).contiguous()
    return out


def integer_case(B, H, W, first_layer, seed):
    """Integer-valued data: saved activations in {0, 1, 2} (about half zero; pooled act = max_pool2d(pre), so positive ties abound),
    image in {0..3}, g_hidden in {-1, 0, 1}, and per layer exactly 8 non-zero weights (+-1) per input channel at seeded (co, tap)
    positions.  backward_reference(..., exact=True) asserts the condition that makes every fp32 sum exact."""
    gen = torch.Generator().manual_seed(seed)
    draw = lambda shape: (torch.randint(0, 4, shape, generator=gen) - 1).clamp_(min=0).float()
    fields = _fields(B, H, W, first_layer, draw)
    weights = {}
    for j, (ci, co) in enumerate(LAYERS):
        at = torch.rand(ci, co * 9, generator=gen).topk(8, dim=1).indices
        sign = (torch.randint(0, 2, (ci, 8), generator=gen) * 2 - 1).float()
        weights[j] = torch.zeros(ci, co * 9).scatter_(1, at, sign).view(ci, co, 3, 3).permute(1, 0, 2, 3).contiguous()
    return {"fields": fields, "weights": weights,
            "image": torch.randint(0, 4, (B, 1, H, W), generator=gen).float(),
            "g_hidden": (torch.randint(0, 3, (B, H // 8, W // 8, 512), generator=gen) - 1).float()}


def real_case(B, H, W, first_layer, seed):
    """Real-valued data: normal weights scaled by 1 / sqrt(9 Cin), saved activations relu(normal) with act = max_pool2d(pre) for the
    pooled layers, normal image and g_hidden"""
    gen = torch.Generator().manual_seed(seed)
    draw = lambda shape: torch.randn(shape, generator=gen).clamp_(min=0)
    fields = _fields(B, H, W, first_layer, draw)
    weights = {j: torch.randn(co, ci, 3, 3, generator=gen) / (9 * ci) ** 0.5 for j, (ci, co) in enumerate(LAYERS)}
    return {"fields": fields, "weights": weights, "image": torch.randn(B, 1, H, W, generator=gen),
            "g_hidden": torch.randn(B, H // 8, W // 8, 512, generator=gen)}


def module_state(weights):
    """a SuperPointNet state dict that holds weights[j] in the eight MFMA layers (the backward reads no other parameter: those are zero)"""
    sd = {"conv1a.weight": torch.zeros(64, 1, 3, 3), "convPb.weight": torch.zeros(65, 256, 1, 1), "convPb.bias": torch.zeros(65),
          "convDb.weight": torch.zeros(256, 256, 1, 1), "convDb.bias": torch.zeros(256), "conv1a.bias": torch.zeros(64)}
    for j, name in enumerate(LAYER_NAMES[:7]):
        sd[f"{name}.weight"], sd[f"{name}.bias"] = weights[j].clone(), torch.zeros(LAYERS[j][1])
    sd["convPa.weight"], sd["convDa.weight"] = weights[7][:256].clone(), weights[7][256:].clone()
    sd["convPa.bias"], sd["convDa.bias"] = torch.zeros(256), torch.zeros(256)
    return sd
