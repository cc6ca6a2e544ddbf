"""Every attention form the default dispatch launches, pinned to float64, with the launched instance asserted.

og_launch_attention (csrc/attention.hip) picks one of many template instances from the shape and from whether the caller passed scratch.
`expected_instance` below restates that rule; every case asserts that the attention instances it launched are exactly the predicted ones,
so a change of the dispatch has to be a deliberate change of this file, and a case cannot drift to another kernel unnoticed.

  a. the stage through ops.attention(return_lse=True) against float64 softmax attention + logsumexp: tile-count edges, both sides of every
     dispatch boundary, spikes that move the running max in the last partial tile and on both sides of the key split's halves, equal and
     large logits, identical keys; key-split results are bit-identical from run to run
  b. strided planes with NaN in the gap columns and a sentinel in the output's gap columns (lib.og_attention directly)
  c. the grid-split forms and their neighbours through SuperGlue against the float64 oracle (og_forward passes scratch)
  d. ragged batches whose small pairs leave key-split halves and grid-split parts without any key tile (og_forward_ragged)
  e. the flash backward at many key blocks, against float64 autograd
"""
import os

import pytest
import torch

from openglue_amd import _lib, ops, synthetic as syn
from oracle import superglue_oracle as orc
from openglue_amd.kernel_trace import attention_instances, launched_kernels
from tests.test_gpu_parity import TOL_SCORES, _build, _index_agreement
from tests.util import MATCH_THRESHOLD, parity_note, to_device

pytestmark = pytest.mark.gpu

# Most dispatch knobs are read once per process: one left in the environment would move every case below to another kernel.
_KNOBS = sorted(k for k in os.environ if k.startswith("OG_ATTN_"))
if _KNOBS:
    raise RuntimeError(f"test_gpu_attention_dispatch runs the default dispatch: unset {_KNOBS}")

# ----------------------------------------------------------------------------- the selection rule, restated
KV_TILE, Q_TILE = 64, 128              # og_common.h
ATTN_COUNTERS = 256                    # og_common.h: OG_ATTN_COUNTERS
ATTN_PARTIAL_WG = 512                  # og_common.h: OG_ATTN_PARTIAL_FLOATS / (4 waves x 34 registers x 64 lanes)


def expected_instance(nz, H, dh, nq, nk, ragged=False, scratch=False):
    """The instance og_launch_attention launches in the default environment: attention.hip, attn_plan restated.  nq: the largest query count of
    the launch, nk: the smallest key count (nqmax / nkmin there); scratch: the caller passed partial + counters (og_forward does)."""
    rd = "RaggedDesc" if ragged else "RaggedNone"
    grid = (nz * H + 7) // 8 * 8 * ((nq + Q_TILE - 1) // Q_TILE)        # attn_plan: wgs
    dma = dh in (32, 64)                                                   # attn_plan: dma
    if dma and scratch and grid <= ATTN_COUNTERS:                          # grid split
        maxwg = 512 if dh == 32 else 256                                   # maxwg
        gs = 1
        if grid * 4 <= maxwg and (ragged or nk >= 16 * KV_TILE):
            gs = 4
        elif grid * 2 <= maxwg and (ragged or nk >= 8 * KV_TILE):
            gs = 2
        if grid * gs > maxwg or grid * gs > ATTN_PARTIAL_WG:               # the two caps
            gs = 1
        if gs > 1:
            return f"attention_dma_kernel<{dh}, {rd}, 1, {gs}, 0, 0>"     # AttnFamily::GSPLIT2 / GSPLIT4
    if dh == 64 and grid <= 256 and (ragged or nk >= 4 * KV_TILE):         # key split (AttnFamily::KSPLIT)
        return f"attention_dma_kernel<64, {rd}, 2, 1, 0, 0>"
    if dh in (16, 128):                                                    # AttnFamily::REG
        return f"attention_kernel<{dh}, {rd}>"
    return f"attention_dma_kernel<{dh}, {rd}, 1, 1, 0, 0>"


def forward_instances(B, m, n, H, dh, ragged=False):
    """The attention instances of one og_forward / og_forward_ragged call (api.hip: self layer = one launch over 2B problems, nq = max,
    nk = min over the two images; cross layer = one launch per side).  m, n: the largest keypoint counts of either image."""
    return {expected_instance(2 * B, H, dh, max(m, n), min(m, n), ragged, True),
            expected_instance(B, H, dh, m, n, ragged, True), expected_instance(B, H, dh, n, m, ragged, True)}


KS64 = "attention_dma_kernel<64, RaggedNone, 2, 1, 0, 0>"
PLAIN64 = "attention_dma_kernel<64, RaggedNone, 1, 1, 0, 0>"


def test_restatement_sides_of_the_boundaries():
    """The boundaries the issue names, as the restatement sees them (a wrong restatement would make every assertion below pointless)."""
    assert expected_instance(8, 4, 64, 1024, 1087) == KS64            # grid.x = 256
    assert expected_instance(8, 4, 64, 1025, 1087) == PLAIN64         # grid.x = 288
    assert expected_instance(2, 4, 64, 129, 255) == PLAIN64
    assert expected_instance(2, 4, 64, 129, 256) == KS64
    assert forward_instances(1, 1024, 1024, 4, 64) == {"attention_dma_kernel<64, RaggedNone, 1, 4, 0, 0>"}
    assert forward_instances(1, 2048, 2048, 4, 32) == {"attention_dma_kernel<32, RaggedNone, 1, 4, 0, 0>"}


@pytest.fixture(scope="module", autouse=True)
def _threads():
    n = torch.get_num_threads()
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))      # float64 references beside the GPU
    yield
    torch.set_num_threads(n)


def _traced(fn):
    """-> (fn's result, the set of attention forward instances it launched, every kernel name in launch order)."""
    box = []
    names = launched_kernels(lambda: box.append(fn()))
    return box[0], attention_instances(names), names


# ----------------------------------------------------------------------------- a. the stage matrix
def _ref(qs, k, v, H):
    """float64 softmax attention on already-scaled q, per problem: -> O [Z, nq, D], lse [Z, H, nq] (natural units)."""
    Z, nq, D = qs.shape
    dh = D // H
    O = torch.empty(Z, nq, D, dtype=torch.float64)
    L = torch.empty(Z, H, nq, dtype=torch.float64)
    for z in range(Z):
        qh, kh, vh = (t[z].double().view(-1, H, dh).transpose(0, 1) for t in (qs, k, v))
        s = qh @ kh.transpose(-1, -2)
        lse = torch.logsumexp(s, -1)
        O[z] = (torch.exp(s - lse[..., None]) @ vh).transpose(0, 1).reshape(nq, D)
        L[z] = lse
    return O, L


FORMS = {          # form -> (H, dh): every form of the first four rows of the dispatch table, at Z = 2 unless the form needs more problems
    "kernel16": (4, 16), "kernel128": (2, 128), "dma32": (4, 32), "dma64": (4, 64), "dma64_ks": (4, 64),
}
NKS = (1, 63, 64, 65, 255, 256, 257, 1087, 2049)
NQS = (1, 127, 129, 1025)


def _z_for(form, nq, nk):
    if form == "dma64" and nk >= 4 * KV_TILE:          # the plain dh-64 kernel at >= 4 key tiles: grid.x > 256
        return 8 if nq > 1024 else 72
    return 2


def _stage_cases():
    out = []
    for form in FORMS:
        for nk in NKS:
            if form == "dma64_ks" and nk < 4 * KV_TILE:
                continue                               # the key split needs >= 4 key tiles
            for nq in NQS:
                out.append((form, nq, nk))
    out += [("boundary", 1024, 1087), ("boundary", 1025, 1087)]      # (Z=8, H=4, dh=64): grid.x = 256 -> key split; 288 -> plain, 17 tiles
    return out


def _run_stage(qs, k, v, H, runs=1):
    dev = torch.device("cuda:0")
    qd, kd, vd = qs.to(dev), k.to(dev), v.to(dev)
    (o, lse), inst, _ = _traced(lambda: ops.attention(qd, kd, vd, H, return_lse=True))
    outs = [(o.cpu(), lse.cpu())]
    for _ in range(runs - 1):
        o2, l2 = ops.attention(qd, kd, vd, H, return_lse=True)
        outs.append((o2.cpu(), l2.cpu()))
    return outs, inst


def _check_stage(tag, qs, k, v, H, want_inst, o_bound):
    dh = qs.shape[2] // H
    ks = want_inst == KS64
    outs, inst = _run_stage(qs, k, v, H, runs=2 if ks else 1)
    assert inst == {want_inst}, (tag, inst, want_inst)
    o, lse = outs[0]
    O, L = _ref(qs, k, v, H)
    err = (o.double() - O).abs().max().item()
    lerr = ((lse.double() - L).abs() - 4e-7 * L.abs()).max().item()
    print(f"[{tag} dh={dh}] {want_inst}: max |O - float64| {err:.2e} (bound {o_bound:.1e}), lse excess {lerr:.2e}")
    assert torch.isfinite(o).all() and torch.isfinite(lse).all(), tag
    assert err < o_bound, (tag, err)
    assert lerr <= 2e-5, (tag, lerr)
    if ks:                                             # the halves merge in a fixed order: run to run bit-identical
        assert torch.equal(outs[1][0], o) and torch.equal(outs[1][1], lse), tag
    return err


@pytest.mark.parametrize("form,nq,nk", _stage_cases())
def test_stage_tile_count_edges(gpu_device, form, nq, nk):
    if form == "boundary":
        Z, (H, dh) = 8, (4, 64)
    else:
        Z, (H, dh) = _z_for(form, nq, nk), FORMS[form]
    want = expected_instance(Z, H, dh, nq, nk)
    if form == "dma64":
        assert want == PLAIN64
    elif form == "dma64_ks":
        assert want == KS64
    g = torch.Generator().manual_seed(nq * 7919 + nk * 31 + dh)
    D = H * dh
    q, k, v = torch.randn(Z, nq, D, generator=g) * 3.0, torch.randn(Z, nk, D, generator=g) * 3.0, torch.randn(Z, nk, D, generator=g) * 2.0
    _check_stage(f"{form} Z={Z} nq={nq} nk={nk}", q * dh ** -0.5, k, v, H, want, 5e-5)


def _set_logit(qs, k, z, i, h, dh, j, target):
    """Key j of problem z becomes the direction of query i (head h), scaled so that logit(i, j) = target."""
    sl = slice(h * dh, (h + 1) * dh)
    qv = qs[z, i, sl]
    k[z, j, sl] = qv * (target / float(qv.double().pow(2).sum()))


def _edge_inputs(kind, Z, H, dh, nq, nk, seed):
    g = torch.Generator().manual_seed(seed)
    D = H * dh
    qs = torch.randn(Z, nq, D, generator=g) * dh ** -0.5          # logits ~ N(0, 1)
    k, v = torch.randn(Z, nk, D, generator=g), torch.randn(Z, nk, D, generator=g)
    nt = (nk + KV_TILE - 1) // KV_TILE
    for z in range(Z):
        for h in range(H):
            if kind == "spike_last":                  # an early max of 15, then one of 30 in the LAST (partial) tile
                i = (5 + h) % nq
                _set_logit(qs, k, z, i, h, dh, 1 % nk, 15.0)
                _set_logit(qs, k, z, i, h, dh, (nt - 1) * KV_TILE + (7 * h + z) % (nk - (nt - 1) * KV_TILE), 30.0)
            elif kind == "spike_halves":              # key split: the max moves in the first tile of the second half, and the other way round
                th = (nt + 1) // 2
                i0, i1 = (9 + h) % nq, (20 + h) % nq
                _set_logit(qs, k, z, i0, h, dh, th * KV_TILE - 1, 15.0)                 # last key of the first half
                _set_logit(qs, k, z, i0, h, dh, min(th * KV_TILE + 3, nk - 1), 30.0)    # first tile of the second half
                _set_logit(qs, k, z, i1, h, dh, th * KV_TILE - 2, 30.0)
                _set_logit(qs, k, z, i1, h, dh, min(th * KV_TILE + 5, nk - 1), 15.0)
            elif kind == "max_at_end":
                _set_logit(qs, k, z, (11 + h) % nq, h, dh, nk - 1, 25.0)
    if kind == "equal":                               # rows whose logits are all equal (0)
        qs[:, 13:17] = 0.0
    elif kind == "large":                             # rows whose logits span about +-80
        for z in range(Z):
            for h in range(H):
                sl = slice(h * dh, (h + 1) * dh)
                for i in range(min(4, nq)):
                    s = (qs[z, i, sl].double() @ k[z, :, sl].double().T).abs().max().item()
                    qs[z, i, sl] *= 80.0 / s
    elif kind == "identical_keys":                    # problem 0: every key the same row (uniform attention), problem 1: half of them
        k[0] = k[0, :1].expand(nk, D).clone()
        k[1, nk // 2:] = k[1, :1]
    return qs, k, v


EDGE_SHAPES = [("kernel16", 2, 4, 16, 129, 1087), ("kernel128", 2, 2, 128, 129, 1087), ("dma32", 2, 4, 32, 129, 1087),
               ("dma64", 2, 4, 64, 129, 255), ("dma64", 8, 4, 64, 1025, 1087), ("dma64_ks", 2, 4, 64, 129, 1087), ("dma64_ks", 2, 4, 64, 129, 257)]
EDGE_KINDS = ("spike_last", "max_at_end", "equal", "large", "identical_keys")


def _edge_cases():
    out = []
    for shp in EDGE_SHAPES:
        for kind in EDGE_KINDS + (("spike_halves",) if shp[0] == "dma64_ks" else ()):
            out.append((*shp, kind))
    return out


@pytest.mark.parametrize("form,Z,H,dh,nq,nk,kind", _edge_cases())
def test_stage_data_edges(gpu_device, form, Z, H, dh, nq, nk, kind):
    want = expected_instance(Z, H, dh, nq, nk)
    assert (want == KS64) == (form == "dma64_ks") and (want == PLAIN64) == (form == "dma64")
    qs, k, v = _edge_inputs(kind, Z, H, dh, nq, nk, seed=nq + nk + dh + len(kind))
    bound = 5e-5 if kind in ("equal", "identical_keys", "max_at_end") else 1e-4 * v.abs().max().item()     # spikes / +-80 logits: the PIPE / P16 bound
    _check_stage(f"{form} {kind} Z={Z} nq={nq} nk={nk}", qs, k, v, H, want, bound)


# ----------------------------------------------------------------------------- b. strided, poisoned planes
@pytest.mark.parametrize("H,dh,nq,nk", [(4, 16, 129, 257), (4, 32, 129, 257), (4, 64, 129, 200), (4, 64, 129, 300), (2, 128, 129, 257)])
def test_strided_planes_ignore_gap_columns(gpu_device, H, dh, nq, nk):
    """ld = D + 64 on q, k, v and O: NaN in the inputs' gap columns must not reach O, the output's gap columns keep their sentinel, and O is
    bit-identical to the compact-layout call.  (4, 64, 129, 200): the plain dh-64 kernel; (4, 64, 129, 300): the key split."""
    lib = _lib.load()
    Z, D = 2, H * dh
    ld = D + 64
    g = torch.Generator().manual_seed(dh + nk)
    dev = gpu_device
    q = (torch.randn(Z, nq, D, generator=g) * 3.0 * dh ** -0.5 * 1.4426950408889634).to(dev)
    k, v = (torch.randn(Z, nk, D, generator=g) * 3.0).to(dev), (torch.randn(Z, nk, D, generator=g) * 2.0).to(dev)
    planes = [p for t in (q, k, v) for p in ops.split_f16(t)]
    st = torch.cuda.current_stream().cuda_stream

    def call(ins, outs, ld_in, ld_out):
        qh, ql, kh, kl, vh, vl = ins
        rc = lib.og_attention(qh.data_ptr(), ql.data_ptr(), ld_in, kh.data_ptr(), kl.data_ptr(), ld_in, vh.data_ptr(), vl.data_ptr(), ld_in,
                              outs[0].data_ptr(), outs[1].data_ptr(), ld_out, Z, nq, nk, H, dh, None, st)
        _lib.check(rc, "og_attention")

    compact = [torch.empty(Z, nq, D, device=dev, dtype=torch.float16) for _ in range(2)]
    _, inst, _ = _traced(lambda: call(planes, compact, D, D))
    want = expected_instance(Z, H, dh, nq, nk)
    assert inst == {want}, (inst, want)
    wide = []
    for p in planes:
        w = torch.full((*p.shape[:2], ld), float("nan"), device=dev, dtype=torch.float16)
        w[..., :D] = p
        wide.append(w)
    sentinel = 12344.0
    owide = [torch.full((Z, nq, ld), sentinel, device=dev, dtype=torch.float16) for _ in range(2)]
    _, inst2, _ = _traced(lambda: call(wide, owide, ld, ld))
    assert inst2 == {want}
    for c, w in zip(compact, owide):
        assert torch.isfinite(w[..., :D]).all()
        assert torch.equal(w[..., :D], c)
        assert (w[..., D:] == sentinel).all()
    O = ops.merge_f16(*compact).cpu().double()
    ref, _ = _ref(q.cpu() / 1.4426950408889634, k.cpu(), v.cpu(), H)
    assert (O - ref).abs().max().item() < 5e-5


# ----------------------------------------------------------------------------- c. grid split and neighbours through og_forward
def _forward_case(D, N, B, stages=2, trained=False, desc_scale=None, seed=11):
    H = 4
    dh = D // H
    cfg = syn.make_config(descriptor_dim=D, num_stages=stages, num_heads=H, num_iters=20, side_info_size=1)
    sd = syn.make_trained_like_state_dict(cfg, seed=0) if trained else syn.make_state_dict(cfg, seed=0)
    model = _build(cfg, sd, torch.device("cuda:0"))
    kw = {} if desc_scale is None else {"desc_scale": desc_scale}
    data = syn.make_batch(B, N, N, D, 1, seed=seed, **kw)
    dd = to_device(data, torch.device("cuda:0"))
    out, inst, _ = _traced(lambda: model.match(dd, MATCH_THRESHOLD))
    want = forward_instances(B, N, N, H, dh)
    assert inst == want, (inst, want)
    out = {k: v.cpu() for k, v in out.items()}
    ndiff, unexplained, o64 = _index_agreement(out["matches0"], out["scores"], sd, cfg, data)
    err = (out["scores"].double() - o64["scores"]).abs().max().item()
    parity_note(f"[attention dispatch D={D} N={N} B={B}{' trained x4' if trained else ''}] {sorted(want)}: scores err {err:.2e} exempt={ndiff}")
    assert torch.isfinite(out["scores"]).all()
    assert err < TOL_SCORES, err
    assert unexplained == 0, (ndiff, unexplained)
    return want


@pytest.mark.parametrize("D,N,B", [(256, 1024, 1), (256, 1024, 2), (256, 1024, 4), (256, 1024, 8), (128, 2048, 1), (128, 2048, 2), (128, 2048, 4)])
def test_forward_grid_split_forms_against_oracle(gpu_device, D, N, B):
    want = _forward_case(D, N, B)
    if (D, B) in ((256, 1), (128, 1)):
        assert any(", 1, 4, 0, 0>" in w for w in want)            # the 4-way grid split is in the sweep
    if (D, B) == (256, 2):
        assert any(", 1, 2, 0, 0>" in w for w in want)


def test_forward_grid_split_on_peaky_attention(gpu_device):
    """A trained-like checkpoint with 4x descriptors (as test_forward_on_trained_like_checkpoint_fixture's x4): peaky attention, so later
    parts of the grid split see maxima that moved; 3 stages at one 1024-keypoint pair (the 4-way grid split everywhere)."""
    want = _forward_case(256, 1024, 1, stages=3, trained=True, desc_scale=4.0, seed=5)
    assert want == {"attention_dma_kernel<64, RaggedNone, 1, 4, 0, 0>"}


# ----------------------------------------------------------------------------- d. ragged batches with empty parts
def _near_ties(s64, gap=1e-4):
    """orc.ambiguous_rows for any shape (a side with a single keypoint has no runner-up)."""
    inner = s64[:, :-1, :-1]

    def amb(dim):
        if inner.shape[dim] < 2:
            return torch.zeros(inner.shape[0], inner.shape[3 - dim], dtype=torch.bool)
        t = inner.topk(2, dim=dim).values
        t = t if dim == 2 else t.transpose(1, 2)
        return (t[..., 0] - t[..., 1]) < gap
    return amb(2), amb(1)


RAGGED = [          # (D, pairs, forms that must run)
    (256, [(1, 1024), (1024, 190)], ("RaggedDesc, 1, 2, 0, 0>", "RaggedDesc, 1, 4, 0, 0>")),
    (256, [(2, 1024), (1024, 63)], ("RaggedDesc, 1, 2, 0, 0>", "RaggedDesc, 1, 4, 0, 0>")),
    (256, [(64, 1024), (1024, 65)], ("RaggedDesc, 1, 2, 0, 0>", "RaggedDesc, 1, 4, 0, 0>")),
    (256, [(1, 1024), (1024, 2), (63, 1024), (1024, 64)], ("RaggedDesc, 2, 1, 0, 0>", "RaggedDesc, 1, 2, 0, 0>")),
    (256, [(65, 1030), (1024, 190), (190, 1024), (1024, 550)], ("RaggedDesc, 2, 1, 0, 0>",)),
    (128, [(1, 1024), (1024, 190)], ("RaggedDesc, 1, 4, 0, 0>",)),
    (128, [(2, 1024), (1024, 63), (64, 1024), (1024, 65)], ("RaggedDesc, 1, 2, 0, 0>", "RaggedDesc, 1, 4, 0, 0>")),
]


@pytest.mark.parametrize("D,lens,forms", RAGGED)
def test_ragged_empty_key_parts(gpu_device, D, lens, forms):
    """Pairs of 1 .. 190 keypoints next to >= 1024: under the ragged key split (<= 64 keys) and grid split (GS = 2: <= 64 keys, GS = 4:
    <= 192) a half or part owns no key tile and must weigh nothing in the merge.  Every pair against the per-pair oracle."""
    H, dh = 4, D // 4
    cfg = syn.make_config(descriptor_dim=D, num_stages=2, num_heads=H, num_iters=20, side_info_size=1)
    sd = syn.make_state_dict(cfg, seed=0)
    dev = torch.device("cuda:0")
    model = _build(cfg, sd, dev)
    pairs_cpu = []
    for i, (m, n) in enumerate(lens):
        p = syn.make_pair(m, n, D, 1, seed=500 + i)
        p["image0_size"] = list(syn.IMAGE_WH); p["image1_size"] = list(syn.IMAGE_WH)
        pairs_cpu.append(p)
    pairs = [to_device(p, dev) for p in pairs_cpu]
    res, inst, _ = _traced(lambda: model.match_ragged(pairs, MATCH_THRESHOLD))
    M, N = max(m for m, _ in lens), max(n for _, n in lens)
    want = forward_instances(len(lens), M, N, H, dh, ragged=True)
    assert inst == want, (inst, want)
    for f in forms:
        assert any(w.endswith(f) for w in want), (f, want)
    worst = 0.0
    for p, r, (m, n) in zip(pairs_cpu, res, lens):
        assert r["scores"].shape == (m + 1, n + 1)
        s = r["scores"].cpu()
        assert torch.isfinite(s).all(), (m, n)
        one = {k: (v[None] if torch.is_tensor(v) else v) for k, v in p.items()}
        with torch.no_grad():
            o64 = orc.superglue_forward(sd, cfg, one, dtype=torch.float64)
        err = (s.double() - o64["scores"][0]).abs().max().item()
        worst = max(worst, err)
        assert err < TOL_SCORES, ((m, n), err)
        ref = orc.extract_matches(o64["scores"].float(), MATCH_THRESHOLD)
        amb_r, amb_c = _near_ties(o64["scores"])
        near_thr = (ref["matching_scores0"] - MATCH_THRESHOLD).abs() < 1e-3
        diff = r["matches0"].cpu()[None] != ref["matches0"]
        for b, i in torch.nonzero(diff).tolist():
            j = int(ref["_row_argmax"][b, i])
            assert bool(amb_r[b, i]) or bool(near_thr[b, i]) or bool(amb_c[b, j]), ((m, n), i)
        assert int(diff.sum()) <= 2, (m, n)
    parity_note(f"[attention dispatch ragged D={D} {lens}] {sorted(want)}: scores err {worst:.2e}")


# ----------------------------------------------------------------------------- e. flash backward at many key blocks
def _bwd_inputs(B, Nq, Nk, H, d):
    g = torch.Generator().manual_seed(Nq * 3 + Nk + d)
    D = H * d
    q, k, v = (torch.randn(B, n_, D, generator=g) for n_ in (Nq, Nk, Nk))
    for b in range(B):
        for h in range(H):              # late spikes: keys in the last (partial) block dominate a few queries
            sl = slice(h * d, (h + 1) * d)
            for i, j in ((3 + h, Nk - 1), (17 + h, Nk - 2 - h), (Nq - 1, (Nk - 1) // 64 * 64)):
                qv = q[b, i % Nq, sl]
                k[b, j, sl] = qv * (12.0 * d ** 0.5 / float(qv.double().pow(2).sum()))
    R = torch.randn(B, Nq, D, generator=g)
    return q, k, v, R


def _bwd_reference(q, k, v, R, H):
    B, Nq, D = q.shape
    d = D // H
    qd, kd, vd = (t.double().requires_grad_(True) for t in (q, k, v))
    qh, kh, vh = (t.reshape(B, -1, H, d).transpose(1, 2) for t in (qd, kd, vd))
    ref = (torch.softmax(qh @ kh.transpose(-1, -2) * d ** -0.5, -1) @ vh).transpose(1, 2).reshape(B, Nq, D)
    (ref * R.double()).sum().backward()
    return ref.detach(), qd.grad, kd.grad, vd.grad


@pytest.mark.parametrize("shape", [(1, 1024, 2049, 4, 64), (2, 129, 1500, 2, 32), (1, 300, 1100, 4, 16)])
def test_flash_backward_many_key_blocks(gpu_device, shape):
    from openglue_amd import train
    B, Nq, Nk, H, d = shape
    dev = gpu_device
    q, k, v, R = _bwd_inputs(B, Nq, Nk, H, d)
    ref, gq, gk, gv = _bwd_reference(q, k, v, R, H)
    qg, kg, vg = (t.to(dev).requires_grad_(True) for t in (q, k, v))
    Rd = R.to(dev)

    def step():
        out = train.SoftmaxAttention.apply(qg, kg, vg, H)
        (out * Rd).sum().backward()
        return out
    out, inst, names = _traced(step)
    assert inst == {expected_instance(B, H, d, Nq, Nk)}, inst
    assert f"attention_bwd_kernel<{d}>" in names, names
    assert not any(n.startswith("attention_lse_kernel<") for n in names), names     # the forward kernel left the lse
    assert (out.detach().cpu().double() - ref).abs().max() < 2e-5
    for name, got, want in (("dq", qg.grad, gq), ("dk", kg.grad, gk), ("dv", vg.grad, gv)):
        err = (got.cpu().double() - want).abs().max() / want.abs().max()
        print(f"[bwd {shape}] {name} rel err {float(err):.2e}")
        assert err < 2e-5, (name, float(err))
    # the same backward when no forward kernel left an lse: _flash_attention_backward computes it (attention_lse_kernel)
    q32, k32, v32 = (t.detach().float().contiguous() for t in (qg, kg, vg))
    (dq, dk, dv), _, names = _traced(lambda: train._flash_attention_backward(q32, k32, v32, out.detach().contiguous(), Rd, H))
    assert f"attention_lse_kernel<{d}>" in names and f"attention_bwd_kernel<{d}>" in names, names
    for name, got, want in (("dq", dq, gq), ("dk", dk, gk), ("dv", dv, gv)):
        err = (got.cpu().double() - want).abs().max() / want.abs().max()
        assert err < 2e-5, (name + " (own lse)", float(err))
