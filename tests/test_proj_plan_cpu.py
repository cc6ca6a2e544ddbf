"""The launch plan of the q | k | v projection (csrc/og_proj_plan.h) WITHOUT a GPU: the header is plain C++, so a small host program includes
it and prints the plan of every request of a sweep, under both policies; the checks compare each plan, step for step, with the restatement
of the routing as it stood before the header existed (tests/proj_plan_ref.py).

The sweep keeps to requests the two callers can make (proj_plan_ref's docstring): og_forward*'s planes are as wide as the matrix, addresses
are multiples of 16 (8 for the stage entry), the copies of the matrix exist where packed_layout / og_proj_block_pack write them.  One
side of one boundary cannot occur alone: plane rows of whole 128-byte lines (ldy % 64 == 0) make the byte offset of EVERY first row a multiple
of 128, so "row offset not a multiple of 128" is reached only together with ldy % 64 != 0 (D = 96 below: the stream kernel is refused by both).
"""
import itertools
import subprocess

import pytest

from openglue_amd import build as og_build, synthetic as syn
from tests import proj_plan_ref as ref
from tests.proj_plan_ref import Forward, Knobs

HARNESS = r"""
#include <cstdio>
#include "og_proj_plan.h"
int main(int argc, char** argv) {
    FILE* f = argc > 1 ? fopen(argv[1], "r") : nullptr;
    if (!f) return 2;
    long long id, row0, rows, split, ldy;
    int policy, a0, a1, b0, b1, K, N, relu_cols, ragged, has_small, has_big, bits, ks, kst, krs, kt, kb2;
    while (fscanf(f, "%lld %d %lld %lld %lld %d %d %d %d %d %d %d %d %d %d %lld %d %d %d %d %d %d", &id, &policy, &row0, &rows, &split, &a0, &a1, &b0, &b1, &K, &N,
                  &relu_cols, &ragged, &has_small, &has_big, &ldy, &bits, &ks, &kst, &krs, &kt, &kb2) == 22) {
        const OgProjRequest q{row0, rows, split, a0, a1, b0, b1, K, N, relu_cols, ragged != 0, has_small != 0, has_big != 0, ldy, (unsigned)bits,
                              OgProjKnobs{ks, kst, krs, kt, kb2}};
        const OgProjPlan p = og_proj_plan(q, policy);
        printf("req %lld %d\n", id, p.n);
        for (int i = 0; i < p.n; ++i) {
            const OgProjStep& s = p.step[i];
            printf("step %d %lld %d %d %d %d %d %d %d\n", s.family, (long long)s.row0, s.rows, s.split_row, s.a0, s.a1, s.b0, s.b1, s.relu);
        }
    }
    return 0;
}
"""
FORWARD, STAGE_ENTRY = 0, 1                     # og_proj_plan.h: OG_PROJ_FORWARD, OG_PROJ_STAGE_ENTRY

PROJ_KNOBS = [Knobs(proj_small=a, proj_stream=b) for a in (-1, 0, 1) for b in (-1, 0, 1, 2)]
GEMM_KNOBS = [Knobs(gemm_row_split=a, gemm_tile=b, gemm_big2=c) for a in (1, 0) for b in (0, 128, 256) for c in (1, 0)]
KNOBS = PROJ_KNOBS + GEMM_KNOBS[1:] + [Knobs(proj_small=0, proj_stream=1, gemm_row_split=0)]

SINGLE_PAIR = [(128, 2048, 1), (128, 1024, 1), (128, 2048, 2), (256, 1024, 1), (128, 700, 3)]      # tests/test_gpu_configs.py: test_single_pair_regime_of_inference_py (D, n, B)


def _shapes():
    """(D, T0, T1, ragged-capable) of the forward sweep."""
    out = [(c["descriptor_dim"], c["batch"] * c["kpts"][0], c["batch"] * c["kpts"][1]) for c in syn.CONFIGS.values()]
    out += [(D, B * n, B * n) for D, n, B in SINGLE_PAIR]
    for D in (64, 96, 128, 192, 256):
        out += [(D, 128, 8064), (D, 128, 8065),                   # T = 8192 / 8193
                (D, 256, 8200), (D, 260, 8200), (D, 96, 8200), (D, 130, 97), (D, 128, 160),          # T0 a multiple of 32 / 128 / 256 and not
                (D, 8320, 8320), (D, 8193, 100), (D, 100, 8193)]
    out += [(256, 12 * 1024, 12 * 1024), (256, 47 * 256, 48 * 256),                 # 192 / 191 big tiles of the row-split GEMM
            (256, 16 * 1024, 16 * 1024), (256, 504 * 32, 512 * 32), (256, 16 * 1024, 16 * 1024 - 5),     # 2048 / 2040 / 2048 units of the row-split launch (T not whole tiles)
            (256, 683 * 16, 683 * 16), (256, 682 * 16, 682 * 16), (256, 682 * 16, 682 * 16 + 1),         # 2049 / 2046 / 2049 units of a self launch
            (256, 32768, 40000), (256, 32736, 40000), (256, 32737, 40000),                                # 2048 / 2046 / 2048 units of the k | v launch
            (256, 512, 65024), (256, 9000, 9000), (256, 2000, 7000)]
    return sorted(set(out))


def _forward_cases():
    """(request line fields, the steps the restatement expects)"""
    cases = []
    for (D, T0, T1), ragged, bits, kn in itertools.product(_shapes(), (False, True), (0, 16, 64), KNOBS):
        for favor in ((False, True) if D == 256 else (False,)):
            f = Forward(D, T0, T1, favor=favor, ragged=ragged, knobs=kn, plane_bits=bits)
            common = (D, f.QW, 2 * f.WQ if favor else 0, int(ragged), int(f.has_small), int(f.has_big), f.QW, bits, *kn)
            cases.append(((FORWARD, 0, f.T, 0, 0, 0, 0, f.QW, *common), f.self_layer()))
            cases.append(((FORWARD, 0, f.T, T0, 0, f.WQ, 0, f.QW, *common), f.cross_side0()))
            cases.append(((FORWARD, 0, T0, 0, 0, 0, f.WQ, f.QW, *common), f.cross_kv()))
            if kn in (Knobs(), Knobs(proj_small=0, proj_stream=1)) and not ragged:
                # ranges that are and are not whole blocks, groups and slabs, at a row offset; one 256-column slab at 2047 / 2048 units
                cols = sorted({0, 16, 32, 96, 128, 256, 384, f.QW - 32, f.QW})
                for r0, R in ((0, T0), (T0, T1), (1, T1), (0, 2047 * 32), (0, 2048 * 32)):
                    for c0, c1 in itertools.combinations(cols, 2):
                        cases.append(((FORWARD, r0, R, 0, 0, 0, c0, c1, *common), f.rows(r0, R, c0, c1)))
    return cases


def _stage_cases():
    cases = []
    for K, M in itertools.product((256, 128), (1, 96, 8192, 8193, 8320, 32768, 65536)):
        for N in (3 * K, 1024, 1152, 3 * K + 32, 2048, 2304):           # 8 / 9 groups: the widest range the stream kernel takes, and one past it
            nb = N // 32
            ranges = [((0, 0), (0, nb)), ((0, K // 32), (0, nb)), ((0, 0), (K // 32, nb)), ((0, 0), (0, nb - 2)), ((0, 0), (4, 12)), ((0, 0), (5, 13)),
                      ((8, 16), (0, 8)), ((0, 0), (0, min(nb, 32))), ((0, 0), (0, min(nb, 36)))]
            for (a, b), ldy, split, bits, mode in itertools.product(ranges, (N, N + 4, N + 8, N + 64), (0, 32, 128, 8192, 8224, M, M + 64), (0, 8, 16, 64),
                                                                    (-1, 0, 1, 2)):
                kn = Knobs(proj_stream=mode)
                line = (STAGE_ENTRY, 0, M, split, 32 * a[0], 32 * a[1], 32 * b[0], 32 * b[1], K, N, 0, 0, 1, int(N % 128 == 0), ldy, bits, *kn)
                cases.append((line, ref.plan_stage_entry(M, K, N, a, b, ldy, split, bits, kn)))
    return cases


@pytest.fixture(scope="module")
def planned(tmp_path_factory):
    """-> {policy: [(request fields, expected steps, the header's steps)]}"""
    d = tmp_path_factory.mktemp("plan")
    src, exe, req = d / "plan.cpp", d / "plan", d / "requests.txt"
    src.write_text(HARNESS)
    subprocess.run([og_build._hipcc(), "-std=c++17", "-O1", "-I", og_build.CSRC, str(src), "-o", str(exe)], check=True, capture_output=True, text=True)
    cases = _forward_cases() + _stage_cases()
    req.write_text("".join(f"{i} {' '.join(str(int(v)) for v in line)}\n" for i, (line, _) in enumerate(cases)))
    got = [None] * len(cases)
    cur = None
    for out in subprocess.run([str(exe), str(req)], check=True, capture_output=True, text=True).stdout.splitlines():
        f = out.split()
        if f[0] == "req":
            cur = got[int(f[1])] = []
        else:
            cur.append((ref.FAMILIES[int(f[1])], *map(int, f[2:])))
    assert all(g is not None for g in got), "the program skipped a request"
    res = {FORWARD: [], STAGE_ENTRY: []}
    for (line, want), g in zip(cases, got):
        res[line[0]].append((line, want, g))
    return res


def _compare(rows):
    bad = [(line, want, got) for line, want, got in rows if [tuple(s) for s in want] != got]
    assert not bad, (len(bad), len(rows), bad[:3])


def test_forward_policy_matches_the_call_sites_it_replaced(planned):
    assert len(planned[FORWARD]) > 10000
    fams = {s[0] for _, _, got in planned[FORWARD] for s in got}
    assert fams == set(ref.FAMILIES), fams                                        # the sweep reaches every family ...
    assert {len(got) for _, _, got in planned[FORWARD]} == {1, 2, 3}              # ... and one, two and three launches per request
    assert any(s[0] == ref.GEMM and s[3] > 0 for _, _, got in planned[FORWARD] for s in got), "no row-split GEMM in the sweep"
    assert any(s[0] == ref.GEMM and s[8] for _, _, got in planned[FORWARD] for s in got), "no favor_relu GEMM in the sweep"
    _compare(planned[FORWARD])


def test_stage_entry_policy_matches_og_proj_block_as_it_was(planned):
    assert len(planned[STAGE_ENTRY]) > 10000
    assert {s[0] for _, _, got in planned[STAGE_ENTRY] for s in got} == {ref.SMALL, ref.WSTAT, ref.STREAM}       # never a GEMM
    assert all(len(got) == 1 for _, _, got in planned[STAGE_ENTRY])
    _compare(planned[STAGE_ENTRY])


def test_the_flagship_requests(planned):
    """C2 (32 pairs x 1024 + 1024 keypoints, 256-d): every request of a stage is ONE proj_wstat launch -- the three launches
    tests/test_proj_wstat_deal_cpu.py: test_the_flagship_launches_fill_the_chip names as (rows, split_row, slabs below, slabs from the split)."""
    c = syn.CONFIGS["C2"]
    T0, T1 = c["batch"] * c["kpts"][0], c["batch"] * c["kpts"][1]

    def plan_of(rows, split, a0, a1, b0, b1):
        line = (FORWARD, 0, rows, split, a0, a1, b0, b1, 256, 768, 0, 0, 1, 0, 768, 0, *Knobs())
        hits = [got for ln, _, got in planned[FORWARD] if tuple(ln) == line]
        assert hits, line
        return hits[0]
    assert plan_of(T0 + T1, 0, 0, 0, 0, 768) == [(ref.WSTAT, 0, 65536, 0, 0, 0, 0, 3, 0)]
    assert plan_of(T0 + T1, T0, 0, 256, 0, 768) == [(ref.WSTAT, 0, 65536, 32768, 0, 1, 0, 3, 0)]
    assert plan_of(T0, 0, 0, 0, 256, 768) == [(ref.WSTAT, 0, 32768, 0, 0, 0, 1, 3, 0)]
    launches = [(s[2], s[3], s[5] - s[4], s[7] - s[6]) for steps in Forward(256, T0, T1).stage() for s in steps]
    assert launches == [(65536, 0, 0, 3), (65536, 32768, 1, 3), (32768, 0, 0, 2)]


def test_new_forward_shapes_cross_the_thresholds_they_are_meant_to():
    """The 256-d batch cases of tests/test_gpu_proj_mlp_forms.py: test_forward_forms, by the restatement."""
    big2, t128 = "gemm_nt_f16x3_big2_kernel<2, 1>", "gemm_nt_f16x3_kernel<128, 2, RaggedNone, 2, 1>"
    f = Forward(256, 12 * 1024, 12 * 1024)               # 2304 units; 1536 units and 192 big tiles; 768 units and 96 big tiles
    assert [[ref.kernel_of(s, 256) for s in r] for r in f.stage()] == [["proj_wstat_kernel"], [big2], [t128]]
    assert f.cross_side0()[0][3] == 12 * 1024
    f = Forward(256, 16 * 1024, 16 * 1024)               # the cross launch: 512 + 1536 = 2048 units
    assert f.cross_side0() == [(ref.WSTAT, 0, 32768, 16384, 0, 1, 0, 3, 0)]
