"""CPU side of the inference-Sinkhorn form tests: the table of tests/sinkhorn_cases.py has the edges it claims, and on every input the
float32 CPU oracle stays so close to float64 that the tight bound of tests/test_gpu_sinkhorn_forms.py (F e32 + 4 ulps) is never the
looser one next to the project's bar."""
import pytest
import torch

from tests import sinkhorn_cases as sc

ORDINARY = sc.ordinary_cases()


def test_the_table_has_every_edge():
    assert {sc.geom(c[2]) for c in sc.PLAIN} == {(1, 4, 1), (2, 4, 1), (4, 2, 1), (4, 2, 2), (4, 2, 4), (8, 1, 4)}
    for lo, hi in ((256, 257), (512, 513), (1024, 1025), (2048, 2049), (4096, 4097)):           # both sides of every sk_geom boundary
        assert sc.geom(lo) != sc.geom(hi) and {lo, hi} <= {c[2] for c in sc.PLAIN}
    assert {c[3] for c in sc.PLAIN} >= {0, 1, 2, 3, 4}
    assert all(c[0] <= 2 and c[3] <= 8 and (c[1] <= 260 or c == sc.PLAIN[14]) for c in sc.PLAIN) and sc.PLAIN[14][1:3] == (2100, 3)
    assert [sc.geom(n) for n in sc.FORCED_N] == [(4, 2, 2), (4, 2, 4), (8, 1, 4)] and all(n % 4 for n in sc.FORCED_N)
    assert len(sc.FORCED) == 21 and all(c[0] == 2 and c[3] == 6 for c in sc.FORCED)
    assert {(r, t) for r, t in sc.FORCED_FORMS} == {(r, t) for r in (32, 64, 128) for t in (0, 1)}
    assert sc.geom(sc.NARROW_IGNORES_OVERRIDES[2])[2] == 1
    B, m, n = sc.AUTO[:3]
    assert (m + 127) // 128 * B >= 512 and B * m * ((n + 3) // 4 * 4) * 4 > 256 << 20 and sc.geom(n) == (4, 2, 2)
    assert all(sc.is_extreme(c) and sc.geom(c[2])[2] > 1 for c in sc.EXTREME) and not any(sc.is_extreme(c) for c in ORDINARY)
    assert sorted((W, rw) for _, _, W, rw in sc.RESIDENT) == [(1, 4), (1, 8), (1, 16), (2, 16), (4, 16)]
    assert [(c[2] + 1023) // 1024 for c in sc.FALLBACK] == [1, 2, 3, 4, 3] and sc.FALLBACK[-1][1] > 16 * 16
    assert all(c[2] % 4 for c, _ in sc.RAW)
    assert [sc.geom(k) for k in sc.RAGGED] == [(1, 4, 1), (4, 2, 1), (4, 2, 2), (4, 2, 4)]
    for nmax, lens in sc.RAGGED.items():
        assert max(n for _, n in lens) == nmax == lens[0][1] and (1, 1) in lens and any(m < 32 for m, _ in lens if m > 1)


def test_inputs_are_seeded_and_spoiled_only_on_the_extreme_rows():
    a, b = sc.make_input(2, 9, 14, sc.SCALE), sc.make_input(2, 9, 14, sc.SCALE)
    assert torch.equal(a, b) and not torch.equal(a, sc.make_input(2, 9, 15, sc.SCALE)[:, :, :14])
    x = sc.make_input(2, 9, 14, 25.0)
    assert bool((x[0, 5] == -100.0).all()) and bool((x[1, :, 7] == 100.0).all())
    assert a.abs().max() < 6 * sc.SCALE


@pytest.mark.parametrize("case", ORDINARY, ids=sc.case_id)
def test_float32_oracle_leaves_room_under_the_cap_ordinary(case):
    _, _, e32, mag = sc.reference(case)
    share = e32 / sc.cap(mag)
    print(f"[sinkhorn cases {sc.case_id(case)}] e32 {e32:.2e} = {100 * share:.1f} % of the cap {sc.cap(mag):.2e}; F e32 = {100 * sc.F_ORDINARY * share:.0f} %")
    assert share <= sc.E32_SHARE_ORDINARY
    assert sc.F_ORDINARY * e32 <= 0.5 * sc.cap(mag)              # the tight bound is never vacuous
    assert sc.tight(case, e32, mag) < sc.cap(mag)


def test_float32_oracle_leaves_room_under_the_cap_automatic_selection_row():
    _, _, e32, mag = sc.reference.__wrapped__(sc.AUTO, sc.AUTO_PAIRS)      # 270 MB of input: not kept
    print(f"[sinkhorn cases {sc.case_id(sc.AUTO)} pairs {sc.AUTO_PAIRS}] e32 {e32:.2e} = {100 * e32 / sc.cap(mag):.1f} % of the cap")
    assert e32 <= sc.E32_SHARE_ORDINARY * sc.cap(mag) and sc.F_ORDINARY * e32 <= 0.5 * sc.cap(mag)


@pytest.mark.parametrize("case", sc.EXTREME, ids=sc.case_id)
def test_float32_oracle_leaves_room_under_the_cap_extreme(case):
    _, ref64, e32, mag = sc.reference(case)
    print(f"[sinkhorn cases {sc.case_id(case)}] e32 {e32:.2e} = {100 * e32 / sc.cap(mag):.1f} % of the cap {sc.cap(mag):.2e}; max |score| {mag:.0f}")
    assert mag > 300                                             # |S / reg|, |u|, |v| of several hundred
    assert e32 <= sc.E32_SHARE_EXTREME * sc.cap(mag)


def test_pairs_of_a_uniform_batch_are_independent_in_the_oracle():
    """What lets the automatic-selection row compute the oracle for three pairs of 64."""
    case = (3, 9, 14, 3, 1.0, 0.7, sc.SCALE)
    _, whole, _, _ = sc.reference(case)
    _, part, _, _ = sc.reference(case, (0, 2))
    assert torch.equal(whole[[0, 2]], part)
