"""The work split of the weight-stationary q | k | v projection (csrc/og_proj_deal.h) WITHOUT a GPU: the header is plain C++, so a small
host program includes it, prints the work of every workgroup for a sweep of (rows, split_row, slabs of the two row ranges), and the
checks run here: every (token block, slab) unit is covered exactly once, no workgroup's run crosses from one row range into the other,
the runs of a range differ by at most one block, and the members of a team share their run and sit on consecutive slots."""
import itertools
import os
import subprocess

import pytest

from openglue_amd import build as og_build

G = 256
HARNESS = r"""
#include <cstdio>
#include <cstdlib>
#include "og_proj_deal.h"
int main(int argc, char** argv) {
    for (int i = 1; i + 3 < argc; i += 4) {
        const int M = atoi(argv[i]), split = atoi(argv[i + 1]), na = atoi(argv[i + 2]), nb = atoi(argv[i + 3]);
        const OgProjDeal d = og_proj_deal_rows(M, split, na, nb, %d);
        printf("case %%d %%d %%d %%d teams %%d %%d\n", M, split, na, nb, d.ta, d.tb);
        for (int id = 0; id < %d; ++id) {
            int range, slab, b0, b1;
            if (og_proj_deal_unit(d, og_proj_deal_slot(id, %d), range, slab, b0, b1))
                printf("wg %%d %%d %%d %%d %%d %%d\n", id, og_proj_deal_slot(id, %d), range, slab, b0, b1);
        }
    }
    return 0;
}
""" % (G, G, G, G)

ROWS = [8193, 8224, 8192 + 32 * 255 + 7, 12000, 16384, 16640, 32768, 65536, 33, 1]
SLABS = [(0, 1), (0, 2), (0, 3), (0, 4), (1, 3), (1, 1), (3, 1), (0, 0), (2, 0)]


def _cases():
    out = []
    for M, (na, nb) in itertools.product(ROWS, SLABS):
        blocks = (M + 31) // 32
        splits = {0, M, M + 64} | {32 * b for b in (1, blocks // 3, blocks // 2, blocks - 1) if 0 < 32 * b < M}
        out += [(M, s, na, nb) for s in sorted(splits)]
    return out


@pytest.fixture(scope="module")
def dealt(tmp_path_factory):
    d = tmp_path_factory.mktemp("deal")
    src, exe = d / "deal.cpp", d / "deal"
    src.write_text(HARNESS)
    subprocess.run([og_build._hipcc(), "-std=c++17", "-O1", "-I", og_build.CSRC, str(src), "-o", str(exe)], check=True, capture_output=True, text=True)
    cases = _cases()
    res = {}
    for i in range(0, len(cases), 64):              # (argument lists stay short)
        args = [str(v) for c in cases[i:i + 64] for v in c]
        cur = None
        for line in subprocess.run([str(exe), *args], check=True, capture_output=True, text=True).stdout.splitlines():
            f = line.split()
            if f[0] == "case":
                cur = res.setdefault(tuple(map(int, f[1:5])), dict(teams=(int(f[6]), int(f[7])), wgs=[]))
            else:
                cur["wgs"].append(tuple(map(int, f[1:])))
    assert set(res) == set(cases)
    return res


def test_header_is_listed_as_a_dependency():
    assert "proj_wstat.hip" in og_build.SOURCES and os.path.exists(os.path.join(og_build.CSRC, "og_proj_deal.h"))


def test_every_unit_once_and_no_run_crosses_a_row_range(dealt):
    for (M, split, na, nb), r in dealt.items():
        tag = (M, split, na, nb)
        blocks = (M + 31) // 32
        ba = 0 if split <= 0 else blocks if split >= M else split // 32
        want = {(b, 0, s) for b in range(ba) for s in range(na)} | {(b, 1, s) for b in range(ba, blocks) for s in range(nb)}
        seen = []
        ids, slots = set(), set()
        for wid, slot, rng, slab, b0, b1 in r["wgs"]:
            assert 0 <= wid < G and 0 <= slot < G and b0 < b1, tag
            ids.add(wid); slots.add(slot)
            lo, hi = (0, ba) if rng == 0 else (ba, blocks)
            assert lo <= b0 and b1 <= hi, (tag, "a run crosses its row range", rng, b0, b1)
            assert 0 <= slab < (na if rng == 0 else nb), tag
            seen += [(b, rng, slab) for b in range(b0, b1)]
        assert len(ids) == len(slots) == len(r["wgs"]), (tag, "slot <-> workgroup id is not one to one")
        assert len(seen) == len(set(seen)), (tag, "a unit is covered twice")
        assert set(seen) == want, (tag, "units missing or invented", len(seen), len(want))


def test_runs_are_even_and_teams_sit_together(dealt):
    for (M, split, na, nb), r in dealt.items():
        tag = (M, split, na, nb)
        ta, tb = r["teams"]
        assert ta * na + tb * nb <= G, tag
        for rng, ns in ((0, na), (1, nb)):
            mine = sorted((slot, slab, b0, b1) for _, slot, g, slab, b0, b1 in r["wgs"] if g == rng)
            if not mine:
                continue
            runs = [b1 - b0 for _, slab, b0, b1 in mine if slab == 0]
            assert max(runs) - min(runs) <= 1, (tag, "uneven runs", runs)
            for i in range(0, len(mine), ns):           # a team: ns consecutive slots, slabs 0 .. ns - 1, ONE run of token blocks
                team = mine[i:i + ns]
                assert [t[1] for t in team] == list(range(ns)), tag
                assert len({t[2:] for t in team}) == 1 and [t[0] for t in team] == list(range(team[0][0], team[0][0] + ns)), tag


def test_the_flagship_launches_fill_the_chip(dealt):
    """C2 (32 pairs x 1024 + 1024 keypoints): the self launch, cross step 1 (q of image 0 + q | k | v of image 1) and cross step 2 (k | v)."""
    longest = lambda k: max(b1 - b0 for *_, b0, b1 in dealt[k]["wgs"])
    assert longest((65536, 0, 0, 3)) == 25 and len(dealt[(65536, 0, 0, 3)]["wgs"]) == 255        # 85 teams of 3: 2048 / 85 = 24.1
    assert longest((65536, 32768, 1, 3)) == 16 and len(dealt[(65536, 32768, 1, 3)]["wgs"]) == 256
    assert longest((32768, 0, 0, 2)) == 8 and len(dealt[(32768, 0, 0, 2)]["wgs"]) == 256
