"""The inference Sinkhorn (csrc/sinkhorn.hip, csrc/sinkhorn_resident.hip) per kernel instance, against orc.matching_log_probs in float64.

sinkhorn_run picks sinkhorn_sweep_kernel<CPL, RG, WPR> and sinkhorn_sweep_fast_kernel<CPL, RG, WPR, ., ROWS, NT> from n, from the number of
workgroups a batch gives and from the size of the score matrices, and og_sinkhorn_resident_wanted moves whole calls to the resident
kernel: every row of tests/sinkhorn_cases.py names the instances it is meant to run and fails if the profiler saw others.

Tolerances (errors are max |got - want| over the scores; every scale comes from the float64 reference, none from the output under test):
  cap    1e-4 + 2e-6 max|ref64|                 the bar of test_sinkhorn_extreme_score_range
  tight  F e32 + 4 * 2^-23 max|ref64|           e32: the float32 CPU oracle's own error on the same input; F from DESIGN.md 4.16;
                                                tests/test_sinkhorn_forms_cpu.py shows F e32 <= half the cap on every ordinary row
  column marginals after any iteration: |logsumexp_rows(scores + norm) - log b| <= cap (log-sum-exp moves by at most the largest
  error of its terms, so this is the score bound again, on a quantity the oracle does not enter)

Instances and the rows that assert them (RD = RaggedNone unless stated):
  sinkhorn_sweep_kernel / sinkhorn_sweep_fast_kernel<., 32, false>, all six geometries     test_streaming_plain
  sinkhorn_sweep_fast_kernel<4,2,2 | 4,2,4 | 8,1,4, ., 32 | 64 | 128, false | true>           test_streaming_forced_rows_and_loads
  <4, 2, 1, ., 32, false> with the overrides set                                          test_narrow_geometry_ignores_the_overrides
  <4, 2, 2, ., 128, true> chosen by sinkhorn_run itself                                    test_streaming_automatic_selection
  sinkhorn_combine_kernel, sinkhorn_combine_fast_kernel, sinkhorn_scores_kernel            every streaming row
  sinkhorn_resident_kernel<1, ., 4 | 8 | 16>, <2, ., 16>, <4, ., 16>                          test_resident_instances
  sinkhorn_fallback_kernel<RaggedNone>                                                     test_fallback_columns_per_thread
  RaggedDesc sweeps of <1,4,1>, <4,2,1>, <4,2,2>, <4,2,4>                                  test_ragged_streaming
"""
import os
import time

import pytest
import torch

from openglue_amd import _lib, ops, synthetic as syn
from openglue_amd.kernel_trace import launched_kernels, sinkhorn_instances
from oracle import superglue_oracle as orc
from tests import sinkhorn_cases as sc
from tests.util import MATCH_THRESHOLD, to_device

pytestmark = pytest.mark.gpu

_KNOBS = ("OG_SINKHORN_RESIDENT", "OG_SK_FAST_ROWS", "OG_SK_FAST_NT", "OG_SINKHORN_FEW", "OG_SINKHORN_FORCE_TIMEOUT", "OG_SINKHORN_AGENT_SCOPE")


@pytest.fixture
def knobs(monkeypatch):
    """-> set(resident, rows=None, nt=None, few=None, timeout=False): the Sinkhorn switches, every one of them stated (sinkhorn_run reads
    them on every call)."""
    assert not os.environ.get("OG_SINKHORN_ROBUST"), "OG_SINKHORN_ROBUST is read once per process and removes the kernels under test"
    for k in _KNOBS:
        monkeypatch.delenv(k, raising=False)

    def set_(resident, rows=None, nt=None, few=None, timeout=False):
        for k, v in (("OG_SINKHORN_RESIDENT", resident), ("OG_SK_FAST_ROWS", rows), ("OG_SK_FAST_NT", nt), ("OG_SINKHORN_FEW", few),
                     ("OG_SINKHORN_FORCE_TIMEOUT", 1 if timeout else None)):
            if v is None:
                monkeypatch.delenv(k, raising=False)
            else:
                monkeypatch.setenv(k, str(v))
    return set_


# ----------------------------------------------------------------------------- which kernels ran
def _targs(name):
    """`kernel<a, b<c, d>, e>` -> ('kernel', ['a', 'b<c, d>', 'e'])"""
    i = name.index("<")
    args, depth, cur = [], 0, ""
    for c in name[i + 1:name.rindex(">")]:
        if c == "," and depth == 0:
            args.append(cur.strip()); cur = ""
            continue
        depth += c in "<(" ; depth -= c in ">)"
        cur += c
    return name[:i], args + [cur.strip()]


def _is_bool(arg, want):
    return arg in (("true", "(bool)1", "1") if want else ("false", "(bool)0", "0"))


def _assert_streaming(inst, n, iters, rows=32, nt=0, rd="RaggedNone"):
    """The streaming schedule of `iters` iterations, launch by launch: the first and the last template arguments are compared, the ragged
    descriptor in between only by its name."""
    heads = [k[:k.index("<")] for k in inst]
    want = (["sinkhorn_sweep_kernel", "sinkhorn_combine_kernel"] if iters else []) + \
        ["sinkhorn_sweep_fast_kernel", "sinkhorn_combine_fast_kernel"] * max(0, iters - 1) + ["sinkhorn_scores_kernel"]
    assert heads == want, inst
    geom = [str(x) for x in sc.geom(n)]
    for k in inst:
        head, a = _targs(k)
        if head == "sinkhorn_sweep_kernel":
            assert a[:3] == geom and len(a) == 4 and a[3].endswith(rd), k
        elif head == "sinkhorn_sweep_fast_kernel":
            assert a[:3] == geom and len(a) == 6 and a[3].endswith(rd) and a[4] == str(rows) and _is_bool(a[5], nt), (k, geom, rows, nt)
        else:
            assert len(a) == 1 and a[0].endswith(rd), k


def _trace(fn, launches, attempts=5):
    """The Sinkhorn launches of fn() in order.  The tracer can lose records: in a run of the whole suite, one or two windows in about 700
    come back with the first 1 to 3 of a call's 13 launches, or with none, on a call whose status word reads 0 and which gives all 13 in
    every other window (a run of this file alone has not shown it).  Records are only ever missing, never added, so a window with fewer
    launches than the schedule has is taken again (fn is repeatable), at most `attempts` times in all, and the last trace is what the
    assertions see, whatever it holds: a schedule that really is short is short every time."""
    for attempt in range(attempts):
        try:
            inst = sinkhorn_instances(launched_kernels(fn))
        except RuntimeError as e:
            if "recorded no device kernel" not in str(e):
                raise
            inst = []
        if len(inst) >= launches:
            break
        print(f"[sk-forms] the tracer reported {len(inst)} of {launches} launches ({inst}), attempt {attempt + 1} of {attempts}")
    return inst


def _run(dev, case, S, launches=None):
    """ops.sinkhorn under the profiler -> (scores on the CPU, status, the Sinkhorn launches in order); `launches`: how many the schedule
    has where it is not the streaming one."""
    _, _, _, iters, reg, z, _ = case
    Sg = S.to(dev)
    box = {}
    inst = _trace(lambda: box.update(r=ops.sinkhorn(Sg, z, iters, reg, return_status=True)), launches or 2 * iters + 1)
    out, status = box["r"]
    return out.cpu(), status, inst


# ----------------------------------------------------------------------------- how far off
def _check(tag, case, got, ref64, e32, mag):
    """Cap, tight bound and column marginals; prints every figure before it asserts."""
    B, m, n, iters = case[:4]
    err = (got.double() - ref64).abs().max().item()
    cap, tight = sc.cap(mag), sc.tight(case, e32, mag)
    line = f"[sk-forms {tag}] err {err:.2e} e32 {e32:.2e} err/e32 {err / e32 if e32 > 0 else float('inf'):.2f} tight {tight:.2e} cap {cap:.2e} (max |score| {mag:.0f})"
    marg = None
    if iters >= 1:
        norm, lb = sc.log_b(m, n)
        marg = (torch.logsumexp(got.double() + norm, dim=1) - lb).abs().max().item()
        line += f" marginals {marg:.2e}"
    print(line)
    assert got.shape == ref64.shape and torch.isfinite(got).all()
    assert err <= cap, (err, cap)
    assert err <= tight, (err, tight)
    assert marg is None or marg <= cap, (marg, cap)
    return err


# ----------------------------------------------------------------------------- streaming schedule
@pytest.mark.parametrize("case", sc.PLAIN, ids=sc.case_id)
def test_streaming_plain(gpu_device, knobs, case):
    knobs(resident=0)
    S, ref64, e32, mag = sc.reference(case)
    got, status, inst = _run(gpu_device, case, S)
    assert status == 0
    _assert_streaming(inst, case[2], case[3])
    _check("plain %s <%d,%d,%d> 32 nt0" % ((sc.case_id(case),) + sc.geom(case[2])), case, got, ref64, e32, mag)


@pytest.mark.parametrize("case", sc.FORCED, ids=sc.case_id)
def test_streaming_forced_rows_and_loads(gpu_device, knobs, case):
    """OG_SK_FAST_ROWS x OG_SK_FAST_NT on the wide geometries: rows per stream, the number of column partials and the stride the combine
    reads them with all change with ROWS; the load hint changes nothing, bit for bit."""
    S, ref64, e32, mag = sc.reference(case)
    outs = {}
    for rows, nt in sc.FORCED_FORMS:
        knobs(resident=0, rows=rows, nt=nt)
        got, status, inst = _run(gpu_device, case, S)
        assert status == 0
        _assert_streaming(inst, case[2], case[3], rows, nt)
        _check("forced %s <%d,%d,%d> %d nt%d" % ((sc.case_id(case),) + sc.geom(case[2]) + (rows, nt)), case, got, ref64, e32, mag)
        outs[rows, nt] = got
    for rows in (32, 64, 128):
        assert torch.equal(outs[rows, 0], outs[rows, 1]), rows        # the same arithmetic in the same order


def test_narrow_geometry_ignores_the_overrides(gpu_device, knobs):
    case = sc.NARROW_IGNORES_OVERRIDES
    S, ref64, e32, mag = sc.reference(case)
    knobs(resident=0, rows=128, nt=1)
    got, status, inst = _run(gpu_device, case, S)
    assert status == 0
    _assert_streaming(inst, case[2], case[3], 32, 0)
    _check("narrow %s overrides ignored" % sc.case_id(case), case, got, ref64, e32, mag)
    knobs(resident=0)
    assert torch.equal(_run(gpu_device, case, S)[0], got)


def test_streaming_automatic_selection(gpu_device, knobs):
    """No override: 64 pairs of 1024 x 1025 give 512 workgroups at 128 rows and 269.5 MB of scores, so sinkhorn_run itself picks
    <4, 2, 2, ., 128, true>.  Pairs of a uniform batch are independent: the oracle runs on three of them."""
    case, pairs = sc.AUTO, list(sc.AUTO_PAIRS)
    t0 = time.time()
    S, ref64, e32, mag = sc.reference.__wrapped__(case, sc.AUTO_PAIRS)
    t1 = time.time()
    knobs(resident=0)
    _, _, _, iters, reg, z, _ = case
    Sg = S.to(gpu_device)
    box = {}
    inst = _trace(lambda: box.update(r=ops.sinkhorn(Sg, z, iters, reg, return_status=True)), 2 * iters + 1)
    out, status = box["r"]
    got = out[pairs].cpu()
    del out, Sg, box
    print(f"[sk-forms auto] input + oracle {t1 - t0:.1f} s, GPU run + copies {time.time() - t1:.1f} s")
    assert status == 0
    _assert_streaming(inst, case[2], iters, 128, 1)
    _check("auto %s pairs %s <4,2,2> 128 nt1" % (sc.case_id(case), pairs), case, got, ref64, e32, mag)


@pytest.mark.parametrize("case", sc.EXTREME, ids=sc.case_id)
def test_streaming_extreme_range_wide_forms(gpu_device, knobs, case):
    """|S / reg|, |u|, |v| of several hundred through the dual-stabilised sweeps of a wide geometry, 32 rows and 128 rows with streaming
    loads: "all terms <= 1, nothing can overflow" (sinkhorn.hip) for the forms that change the rows per stream."""
    S, ref64, e32, mag = sc.reference(case)
    for rows, nt in sc.EXTREME_FORMS:
        knobs(resident=0, rows=rows, nt=nt)
        got, status, inst = _run(gpu_device, case, S)
        assert status == 0
        _assert_streaming(inst, case[2], case[3], rows, nt)
        _check("extreme %s <4,2,2> %d nt%d" % (sc.case_id(case), rows, nt), case, got, ref64, e32, mag)


# ----------------------------------------------------------------------------- resident schedule and its safety net
@pytest.mark.parametrize("row", sc.RESIDENT, ids=lambda r: "%s-few%s-W%d-rw%d" % (sc.case_id(r[0]), r[1], r[2], r[3]))
def test_resident_instances(gpu_device, knobs, row):
    case, few, W, rw = row
    S, ref64, e32, mag = sc.reference(case)
    knobs(resident=2, few=few)
    got, status, inst = _run(gpu_device, case, S, launches=5)
    heads = [k[:k.index("<")] for k in inst]
    # iteration 1 streamed, iterations 2 .. iters in one resident launch, the safety net behind it (returns at once), the scores
    assert heads == ["sinkhorn_sweep_kernel", "sinkhorn_combine_kernel", "sinkhorn_resident_kernel", "sinkhorn_fallback_kernel", "sinkhorn_scores_kernel"], inst
    _, a = _targs(inst[2])
    assert len(a) == 3 and a[0] == str(W) and a[1].endswith("RsUniform") and a[2] == str(rw), inst[2]
    assert status == 0
    _check("resident %s <%d, RsUniform, %d>" % (sc.case_id(case), W, rw), case, got, ref64, e32, mag)


@pytest.mark.parametrize("case", sc.FALLBACK, ids=sc.case_id)
def test_fallback_columns_per_thread(gpu_device, knobs, case):
    """OG_SINKHORN_FORCE_TIMEOUT=1 sets the status word instead of launching the resident kernel; the safety net then solves the pair again,
    one workgroup of 1024 threads per pair: columns tid, tid + 1024, ... up to four per thread, rows 16 at a time."""
    S, ref64, e32, mag = sc.reference(case)
    knobs(resident=2, timeout=True)
    got, status, inst = _run(gpu_device, case, S, launches=4)
    heads = [k[:k.index("<")] for k in inst]
    assert heads == ["sinkhorn_sweep_kernel", "sinkhorn_combine_kernel", "sinkhorn_fallback_kernel", "sinkhorn_scores_kernel"], inst
    _, a = _targs(inst[2])
    assert len(a) == 1 and a[0].endswith("RaggedNone"), inst[2]
    assert status == 2
    _check("fallback %s %d columns per thread" % (sc.case_id(case), (case[2] + 1023) // 1024), case, got, ref64, e32, mag)


# ----------------------------------------------------------------------------- the raw ABI on the streaming schedule
def _r4(x):
    return (x + 3) // 4 * 4


class _Raw:
    """og_sinkhorn on caller-owned buffers."""

    def __init__(self, dev, case):
        self.dev, self.case = dev, case
        B, m, n = case[:3]
        self.nbytes = _lib.load().og_sinkhorn_workspace_bytes(B, m, n)
        assert self.nbytes > 0

    def pad(self, S, lds, fill):
        B, m, n = self.case[:3]
        buf = torch.full((B, m, lds), fill, dtype=torch.float32)
        buf[:, :, :n] = S
        return buf.to(self.dev)

    def run(self, Sp, wp):
        B, m, n, iters, reg, z, _ = self.case
        scores = torch.full((B, m + 1, n + 1), float("nan"), device=self.dev)          # the sentinel: whatever is not overwritten stays NaN
        _lib.call("og_sinkhorn", self.dev, Sp.data_ptr(), Sp.shape[2], float(z), B, m, n, iters, float(reg), scores.data_ptr(), wp, _lib.STREAM)
        torch.cuda.synchronize()
        return scores.cpu()


@pytest.mark.parametrize("row", sc.RAW, ids=lambda r: sc.case_id(r[0]) + ("" if r[1] is None else "-rows%d-nt%d" % r[1]))
def test_streaming_raw_abi(gpu_device, knobs, row):
    """What only the C entry point reaches on the streaming schedule: lds > n with non-finite gap columns (the fast sweep loads v and S in
    groups of four and stores partials for columns >= n), and a workspace that a larger call has used and that then holds NaN everywhere."""
    case, form = row
    B, m, n, iters, reg, z, scale = case
    assert n % 4
    rows, nt = form if form else (None, None)
    knobs(resident=0, rows=rows, nt=nt)
    S, ref64, e32, mag = sc.reference(case)
    raw = _Raw(gpu_device, case)
    ws, wp = _lib.workspace(raw.nbytes, gpu_device)
    S0 = raw.pad(S, _r4(n), 0.0)
    box = {}
    inst = _trace(lambda: box.update(r=raw.run(S0, wp)), 2 * iters + 1)
    plain = box["r"]
    _assert_streaming(inst, n, iters, *(form if form and sc.geom(n)[2] > 1 else (32, 0)))
    _check("raw %s plain %s" % (sc.case_id(case), form), case, plain, ref64, e32, mag)
    lds = _r4(n) + 8
    for fill in (0.0, float("nan")):
        assert torch.equal(raw.run(raw.pad(S, lds, fill), wp), plain), fill
    # a workspace a LARGER call has used, then all-ones bytes (NaN as float): nothing of it may be read before it is written
    big_case = sc._c(B + 1, m + 9, n + 64, iters, reg, z, scale)
    big = _Raw(gpu_device, big_case)
    Sb = sc.make_input(B + 1, m + 9, n + 64, scale)
    wsb, wpb = _lib.workspace(big.nbytes, gpu_device)
    assert big.nbytes >= raw.nbytes
    assert torch.isfinite(big.run(big.pad(Sb, _r4(n + 64), 0.0), wpb)).all()
    assert torch.equal(raw.run(S0, wpb), plain)
    wsb.fill_(255)
    assert torch.equal(raw.run(S0, wpb), plain)
    assert torch.equal(raw.run(raw.pad(S, lds, float("nan")), wpb), plain)
    assert _lib.load().og_sinkhorn_status(wpb, B, m, n) == 0
    del ws, wsb


# ----------------------------------------------------------------------------- ragged streaming (RaggedDesc instances)
@pytest.mark.parametrize("nmax", sorted(sc.RAGGED, reverse=True))
def test_ragged_streaming(gpu_device, knobs, nmax):
    """model.match_ragged on the streaming schedule: the sweeps are the RaggedDesc instances of the widest pair's geometry class with 32
    rows and plain loads, and every pair equals the per-pair float64 oracle, the 1 x 1 pair and the one of fewer than 32 rows included."""
    from openglue_amd.superglue import SuperGlue
    knobs(resident=0, rows=128, nt=1)                      # the overrides are for uniform batches only
    lens = sc.RAGGED[nmax]
    cfg = syn.make_config(descriptor_dim=64, num_stages=1, num_heads=4, num_iters=sc.RAGGED_ITERS, side_info_size=1)
    sd = syn.make_state_dict(cfg, seed=0)
    model = SuperGlue(cfg).eval()
    model.load_state_dict(sd, strict=True)
    model.to(gpu_device)
    pairs_cpu = []
    for i, (m, n) in enumerate(lens):
        p = syn.make_pair(m, n, 64, 1, seed=300 + nmax + i)
        p["image0_size"] = list(syn.IMAGE_WH); p["image1_size"] = list(syn.IMAGE_WH)
        pairs_cpu.append(p)
    dev_pairs = [to_device(p, gpu_device) for p in pairs_cpu]
    # the model's workspace first serves four pairs of the widest size, which write the column partials of every row block: a smaller pair
    # of the call under test that merged more row blocks than it owns would pick those up
    model.match_ragged([dev_pairs[0]] * len(lens), MATCH_THRESHOLD)
    box = {}
    inst = _trace(lambda: box.update(r=model.match_ragged(dev_pairs, MATCH_THRESHOLD)), 2 * sc.RAGGED_ITERS + 1)
    assert model.check_status() == 0
    _assert_streaming(inst, nmax, sc.RAGGED_ITERS, 32, 0, rd="RaggedDesc")
    for p, r, (m, n) in zip(pairs_cpu, box["r"], lens):
        one = {k: (v[None] if torch.is_tensor(v) else v) for k, v in p.items()}
        with torch.no_grad():
            ref = orc.match_pairs(sd, cfg, one, MATCH_THRESHOLD, dtype=torch.float64)
        assert r["scores"].shape == (m + 1, n + 1)
        err = (r["scores"].cpu().double() - ref["scores"][0]).abs().max().item()
        print(f"[sk-forms ragged n_max {nmax} pair {m}x{n}] scores err {err:.2e} (bar 1e-3)")
        assert torch.isfinite(r["scores"]).all() and err < 1e-3
