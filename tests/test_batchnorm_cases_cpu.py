"""CPU side of the train-mode BatchNorm tests: the cases of tests/batchnorm_cases.py have what they claim, float32 arithmetic can meet every
bound the GPU tests use, and the numpy restatement of the forward's statistics passes shows what the per-lane pivots are for."""
import numpy as np
import pytest
import torch

from tests import batchnorm_cases as bc

IDS = [bc.case_name(c) for c in bc.CASES]
QUANTITIES = ("y", "mean", "invstd", "running_mean", "running_var", "dz", "dweight", "dbias")


def test_the_case_table_has_every_edge():
    shapes = {(r, c) for r, c, _, _ in bc.CASES}
    assert shapes == {(1, 4), (2, 4), (3, 8), (31, 36), (32, 64), (33, 260), (150, 512), (1000, 132), (4099, 256)}
    assert {p for _, _, p, _ in bc.CASES} == {0, 4, 8}
    nblk = lambda r: (r + bc.ROWS_PER_BLOCK - 1) // bc.ROWS_PER_BLOCK
    assert [nblk(r) for r, _, _, _ in bc.CASES] == [1, 1, 1, 1, 1, 2, 5, 32, 129]
    assert 1000 % 32 and 4099 % 32 and 129 % 4 and 260 % 256 == 4


@pytest.mark.parametrize("case", bc.CASES, ids=IDS)
def test_census(case):
    """Every case has what its row of the table claims."""
    k = bc.make_case(*case)
    assert k.z.shape == k.a.shape == k.dy.shape == (k.rows, k.C) and k.z.dtype == torch.float32
    assert torch.equal(torch.relu(k.z.double()), k.a.double())                     # relu(z64) == a exactly
    assert not bool(((k.a > 0) & (k.a < 1e-6)).any())                              # the mask is never a rounding question
    assert bool((k.dy != 0).all()) and bool(k.running_mean.abs().min() > 0) and bool((k.running_var - 1).abs().min() > 0)
    assert bool((k.weight < 0).any()) or k.C == 4
    ordinary = bc.ordinary_channels(k.C)
    act = (k.a[:, ordinary] > 0)
    if k.rows >= 2:
        assert bool(act.any(0).all()) and bool((~act).any(0).all())                # both branches of the mask in every ordinary channel
    else:
        assert bool(act.any()) and bool((~act).any())
    if k.rows >= 100:                                                              # roughly half zero after the ReLU
        assert 0.4 < float(act.float().mean()) < 0.6
    if k.C >= 8:
        assert bool((k.z[:, bc.DEAD] < 0).all()) and bool((k.a[:, bc.DEAD] == 0).all())
        assert bool((k.a[:, bc.CONST] == bc.CONST_VALUE).all())
        off = k.a[:, bc.OFFSET].double()
        assert abs(float(off.mean()) - 10.0) < 2e-2 and float(off.max() - off.min()) < 0.1
        zero = k.a[:, bc.SPARSE] == 0
        assert bool(zero.any()) and bool((~zero).any()) and bool((k.z[:, bc.SPARSE][zero] == 0).all())   # the ReLU tie
        assert bool((k.dy[:, bc.SPARSE][zero] != 0).all())                         # exact zeros that receive a gradient
        if k.rows >= 100:
            assert 0.8 < float(zero.float().mean()) < 0.97
    else:
        assert bc.special_channels(k.C) == ()


def test_padded_layout():
    t = torch.arange(6.0).reshape(2, 3)
    p = bc.padded(t, 5, float("nan"))
    assert p.shape == (2, 5) and torch.equal(p[:, :3], t) and bool(torch.isnan(p[:, 3:]).all())


def test_reference_is_the_oracle_under_autograd():
    """The reference's y and running statistics are oracle.batchnorm_train's; its gradients are autograd's of relu + that; at one row the
    running variance takes the biased variance (0)."""
    k = bc.make_case(1, 4, 4, 0)
    r = bc.reference(k)
    assert torch.equal(r["running_var"], (1 - bc.MOMENTUM) * k.running_var.double())
    assert torch.equal(r["y"][0], k.bias.double()) and torch.equal(r["mean"], k.a[0].double())
    k = bc.make_case(33, 260, 4, 0)
    r = bc.reference(k)
    a = k.a.double()
    assert (r["running_var"] - (0.9 * k.running_var.double() + 0.1 * a.var(0, unbiased=True))).abs().max() < 1e-14
    want = torch.nn.functional.batch_norm(a, None, None, k.weight.double(), k.bias.double(), True, 0.1, bc.EPS)
    assert (r["y"] - want).abs().max() < 1e-9
    m = bc.reference(k, relu_mask=0)
    assert torch.equal(m["dweight"], r["dweight"]) and torch.equal(m["dz"] * (a > 0), r["dz"])
    assert bool((r["dz"][k.a == 0] == 0).all()) and bool((m["dz"][k.a == 0] != 0).any())


@pytest.mark.parametrize("case", bc.CASES, ids=IDS)
def test_float32_cpu_attains_every_bound(case):
    """The same formulas in float32 on the CPU stay inside every bound, with and without the ReLU mask: the bounds ask for nothing that
    float32 arithmetic cannot deliver."""
    k = bc.make_case(*case)
    for relu_mask in (1, 0):
        r64 = bc.reference(k, relu_mask)
        r32 = bc.reference(k, relu_mask, dtype=torch.float32)
        bnd = bc.bounds(k, r64)
        worst = {q: bc.ratio(r32[q], r64[q], bnd[q]) for q in QUANTITIES}
        print(f"[float32 cpu {bc.case_name(case)} mask {relu_mask}] " + " ".join(f"{q} {v:.2f}" for q, v in worst.items()))
        assert all(v <= 1.0 for v in worst.values()), worst


# ------------------------------------------------------------------------------------------------------------------
# the statistics passes in numpy
@pytest.mark.parametrize("case", bc.CASES, ids=IDS)
def test_emulation_on_the_cases(case):
    """The kernel's scheme, restated, meets the bars of mean and invstd on every case: ragged slabs, empty waves, dead and constant channels."""
    k = bc.make_case(*case)
    mean, invstd = bc.emulate_stats(k.a.numpy())
    m64, _, _ = bc.stats64(k.a)
    assert np.abs(mean - m64).max() < bc.MEAN_BAR
    assert bc.invstd_error(invstd, k.a).max() < bc.INVSTD_BAR
    if k.C >= 8:
        assert invstd[bc.DEAD] == invstd[bc.CONST] == np.float32(1.0 / np.sqrt(np.float64(np.float32(bc.EPS))))
        assert mean[bc.DEAD] == 0 and mean[bc.CONST] == np.float32(bc.CONST_VALUE)


def test_emulation_row0_shift_loses_the_variance():
    """A channel-wide shift by ROW 0 (the scheme pass 1 had) protects against cancellation only while row 0 is typical of its channel: with
    a ReLU zero there the sums run unshifted.  The worst of 16 channels at 65536 rows, within a factor of two of what was predicted:
        10 +- 1e-2: 1.2e-4    10 +- 1e-3: 5.2e-4    10 +- 1e-4: 7.2e-4    1000 +- 1: 1.1e-4       (bar: 1e-4)
    at 8192 and 1000 rows it stays below the bar (the effect grows with the row count), with a typical row 0 below 1e-6.
    The per-lane pivots with Chan's merge (emulate_stats) stay below 1e-6 on every one of these inputs."""
    for (centre, spread), predicted in bc.ROW0_TABLE:
        x = bc.table_input(centre, spread)
        old = bc.invstd_error(bc.emulate_stats_row0_shift(x)[1], x).max()
        new = bc.invstd_error(bc.emulate_stats(x)[1], x).max()
        print(f"[emulation {centre:g} +- {spread:g}, row 0 = 0] row-0 shift {old:.2e} (predicted {predicted:.1e}); per-lane pivots {new:.2e}")
        assert predicted / 2 <= old <= predicted * 2
        assert new < 1e-6
    last = None
    for rows, _ in reversed(bc.ROW0_TABLE_ROWS):
        x = bc.table_input(10.0, 1e-2, rows=rows)
        old = bc.invstd_error(bc.emulate_stats_row0_shift(x)[1], x).max()
        print(f"[emulation 10 +- 0.01, row 0 = 0, {rows} rows] row-0 shift {old:.2e}")
        assert old < bc.INVSTD_BAR and (last is None or old > last)
        last = old
    x = bc.table_input(10.0, 1e-3, row0_zero=False)
    assert bc.invstd_error(bc.emulate_stats_row0_shift(x)[1], x).max() < 1e-6
    assert bc.invstd_error(bc.emulate_stats(x)[1], x).max() < 1e-6


def test_emulation_row0_case():
    """The 65536 x 256 case of the GPU test, first 40 channels: the row-0 shift misses the invstd bar on channels 0-15 (5.7e-4), the
    kernel's scheme meets it on every channel with two orders to spare; the mean meets 1e-5 either way."""
    x = bc.row0_case().numpy()[:, :40]
    m64, _, _ = bc.stats64(x)
    old = bc.invstd_error(bc.emulate_stats_row0_shift(x)[1], x)
    mean, invstd = bc.emulate_stats(x)
    new = bc.invstd_error(invstd, x)
    print(f"[emulation row-0 case] row-0 shift: ch 0-15 {old[:16].max():.2e}, 16-31 {old[16:32].max():.2e}; per-lane pivots: ch 0-15 "
          f"{new[:16].max():.2e}, 16-31 {new[16:32].max():.2e}, Gaussian {new[32:].max():.2e}; mean {np.abs(mean - m64).max():.2e}")
    assert old[:16].max() > bc.INVSTD_BAR and old[16:].max() < 1e-6
    assert new.max() < 1e-6
    assert np.abs(mean - m64).max() < bc.MEAN_BAR


# ------------------------------------------------------------------------------------------------------------------
# the inputs of the autograd-node tests
@pytest.mark.parametrize("case", bc.MLP_CASES, ids=[bc.mlp_name(c) for c in bc.MLP_CASES])
def test_mlp_cases_keep_clear_of_relu_ties_and_float32_attains_the_bound(case):
    T, splits, sizes, seed = case
    x, params, buffers, R = bc.make_mlp_case(*case)
    r64 = bc.mlp_reference(x, params, buffers, R, splits)
    assert r64["min_preact"] > bc.MLP_MIN_PREACT
    r32 = bc.mlp_reference(x, params, buffers, R, splits, dtype=torch.float32)
    for k, want in r64.items():
        if k == "min_preact":
            continue
        bound = bc.MEAN_BAR if "running" in k else bc.mlp_bound(want, T, sizes, k == "y")
        assert float((r32[k].double() - want).abs().max()) <= bound, k


def test_mlp_reference_row_ranges_matter():
    """(37, 91), (91, 37) and one range give three different outputs and running statistics: a node that ignored `splits` passes one."""
    T, _, sizes, seed = bc.MLP_CASES[0]
    x, params, buffers, R = bc.make_mlp_case(T, None, sizes, seed)
    runs = [bc.mlp_reference(x, params, buffers, R, s) for s in ((37, 91), (91, 37), None)]
    for i in range(3):
        for j in range(i + 1, 3):
            for k in ("y", "grad_x", "grad_2.weight", "2.running_mean", "2.running_var"):
                want = runs[i][k]
                bound = bc.MEAN_BAR if "running" in k else bc.mlp_bound(want, T, sizes, k == "y")
                assert float((runs[j][k] - want).abs().max()) > 20 * bound, (i, j, k)
