"""The table of the inference-Sinkhorn tests (csrc/sinkhorn.hip, csrc/sinkhorn_resident.hip): every row names the kernel instances it
is meant to run.  Plain torch on the CPU; tests/test_sinkhorn_forms_cpu.py checks the inputs, tests/test_gpu_sinkhorn_forms.py runs them.

A case is (B, m, n, iters, reg, dustbin, input scale); scale 4 rows are ordinary, the extreme rows (any other scale) carry the spoiled row
and column of test_sinkhorn_extreme_score_range.  The reference is orc.matching_log_probs in float64; the same call in float32 on the CPU gives
e32 = max |ref32 - ref64| of that input, the yardstick of the tight bound:

  cap    err <= 1e-4 + 2e-6 max|ref64|                      the project's bar (test_sinkhorn_extreme_score_range, _check_scores)
  tight  err <= F e32 + 4 * 2^-23 max|ref64|                F_ORDINARY / F_EXTREME below; DESIGN.md 4.16 has the measurements behind them
  and, so that the tight bound is never the looser one: F e32 <= 0.5 cap on every ordinary row (asserted on the CPU over the whole table)
"""
from __future__ import annotations

import math
from functools import lru_cache

import torch

from oracle import superglue_oracle as orc

SCALE = 4.0
# Twice the largest err / e32 measured on the MI355X over the rows of each kind, rounded up to a power of two (1.94 over
# the ordinary rows, 0.94 over the extreme ones).
F_ORDINARY = 4.0
F_EXTREME = 2.0
ULP_TERM = 4 * 2.0 ** -23
E32_SHARE_ORDINARY, E32_SHARE_EXTREME = 0.05, 0.3      # of the cap: what the CPU test asks of every input


# Inputs whose float32 oracle missed its share of the cap with the plain seed (5.4 % on this one) take the next seed that meets it.
RESEED = {(2, 129, 2049, SCALE): 3}


def geom(n):
    """sk_geom: n -> the <CPL, RG, WPR> of both sweeps."""
    if n <= 256: return (1, 4, 1)
    if n <= 512: return (2, 4, 1)
    if n <= 1024: return (4, 2, 1)
    if n <= 2048: return (4, 2, 2)
    if n <= 4096: return (4, 2, 4)
    return (8, 1, 4)


def is_extreme(case) -> bool:
    return case[6] != SCALE


def case_id(case) -> str:
    return "B%d-%dx%d-it%d-reg%g-z%g-x%g" % tuple(case)


def make_input(B, m, n, scale):
    """randn * scale from a generator seeded by the shape, as _inputs of tests/test_gpu_sinkhorn_train.py; scale != 4: a row nobody wants and
    a column everybody wants."""
    g = torch.Generator().manual_seed(B * 1000003 + m * 4099 + n * 17 + int(scale * 10) + 7919 * RESEED.get((B, m, n, scale), 0))
    S = torch.randn(B, m, n, generator=g) * scale
    if scale != SCALE:
        S[0, 5, :] = -4.0 * scale
        S[-1, :, 7] = 4.0 * scale
    return S


def oracle(S, z, iters, reg, dtype):
    return orc.matching_log_probs(S.to(dtype), torch.tensor(z, dtype=dtype), iters, reg)


@lru_cache(maxsize=None)
def reference(case, pairs=None):
    """-> (S float32 [B, m, n], ref64 of the pairs, e32, max|ref64|); `pairs` (a tuple of batch indices) restricts the oracle to those
    pairs of a uniform batch, which are independent.  Computed once per case and shared: treat as read-only."""
    B, m, n, iters, reg, z, scale = case
    S = make_input(B, m, n, scale)
    Sr = S if pairs is None else S[list(pairs)]
    ref64 = oracle(Sr, z, iters, reg, torch.float64)
    e32 = (oracle(Sr, z, iters, reg, torch.float32).double() - ref64).abs().max().item()
    return S, ref64, e32, ref64.abs().max().item()


def cap(mag) -> float:
    return 1e-4 + 2e-6 * mag


def tight(case, e32, mag) -> float:
    return (F_EXTREME if is_extreme(case) else F_ORDINARY) * e32 + ULP_TERM * mag


def log_b(m, n):
    """log column marginals + norm: what logsumexp(scores + norm, rows) equals after any v update."""
    norm = -math.log(m + n)
    lb = torch.full((n + 1,), norm, dtype=torch.float64)
    lb[-1] += math.log(m)
    return norm, lb


def _c(B, m, n, iters, reg=1.0, z=0.7, scale=SCALE):
    return (B, m, n, iters, float(reg), float(z), float(scale))


# ---- streaming schedule (OG_SINKHORN_RESIDENT=0), 32 rows per workgroup, plain loads ----
# one row per geometry and the other side of every sk_geom boundary; m = 33 + n % 7 as EDGES of the training test: two row blocks, the
# second one nearly empty.  4 iterations = the max-subtracted one and all three unit conversions of the dual-stabilised ones
# (natural -> base 2, base 2 -> base 2, base 2 -> natural).
BOUNDARY_N = (255, 256, 257, 512, 513, 1024, 1025, 2048, 2049, 4096, 4097, 8192)
PLAIN = [_c(1 + (n % 2), 33 + n % 7, n, 4) for n in BOUNDARY_N] + [
    _c(1, 1, 1, 3),
    _c(1, 1, 4097, 3),                     # one row, the widest geometry
    _c(1, 2100, 3, 3),                     # 66 row blocks: the combine merges them in chunks of 8 (8 full chunks + 2)
    _c(2, 37, 200, 0),                     # only the scores kernel
    _c(2, 37, 200, 1),                     # the max-subtracted iteration alone
    _c(2, 37, 200, 2),                     # one dual-stabilised iteration: natural units in and out
    _c(2, 37, 200, 7),
    _c(2, 260, 300, 5, reg=0.7, z=-0.5),   # 9 row blocks: one past a chunk of the combine
    _c(1, 129, 1025, 6),
    _c(1, 200, 2049, 6, reg=0.8),
    _c(1, 130, 4097, 4),
    _c(1, 257, 8192, 3),
]

# ---- forced rows per workgroup and load hint: (OG_SK_FAST_ROWS, OG_SK_FAST_NT) at the three wide geometries ----
FORCED_N = (1025, 2049, 4097)              # <4,2,2>, <4,2,4>, <8,1,4>; n % 4 != 0
FORCED_M = (1, 63, 64, 65, 128, 129, 200)  # one row, a partial stream, an exact stream (of 64 rows at WPR 2), a stream with one live row, an
                                           # exact workgroup, a second workgroup holding one row, two uneven workgroups
FORCED_FORMS = ((32, 0), (32, 1), (64, 0), (64, 1), (128, 0), (128, 1))       # (32, 0) is what runs unforced: the baseline of the comparison
FORCED = [_c(2, m, n, 6) for n in FORCED_N for m in FORCED_M]
NARROW_IGNORES_OVERRIDES = _c(2, 65, 1000, 6)     # WPR == 1: rows = 128, NT = 1 asked, <4, 2, 1, ., 32, false> runs

# ---- automatic selection: 8 * 64 = 512 workgroups at 128 rows, 64 * 1024 * 1028 * 4 bytes = 269.5 MB > 256 MB ----
AUTO = _c(64, 1024, 1025, 2)
AUTO_PAIRS = (0, 31, 63)

# ---- extreme range at a wide geometry: the two extreme rows of the training table.  The second one runs 15 iterations instead of 30: at
# 1100 columns the float32 oracle is 31 to 43 % of the cap away from float64 after 30 (16 seeds), 21 to 22 % after 15 ----
# The third row is the second with one row more: m % 32 != 0 leaves rows >= m in the last workgroup of the 32-row form as well, and with
# (z / reg + v_N) log2(e) near -426 their dustbin term underflows (this is the input on which those rows once put NaN into the column sums).
EXTREME = [_c(2, 96, 1100, 30, reg=0.5, z=0.7, scale=25.0), _c(2, 96, 1100, 15, reg=0.1, z=-30.0, scale=8.0),
           _c(2, 97, 1100, 15, reg=0.1, z=-30.0, scale=8.0)]
EXTREME_FORMS = ((32, 0), (128, 1))

# ---- resident schedule (OG_SINKHORN_RESIDENT=2): case, OG_SINKHORN_FEW, tile width W, rows per wave ----
RESIDENT = [
    (_c(1, 129, 1000, 6), "1", 1, 4),
    (_c(1, 129, 1000, 6), "8", 1, 8),
    (_c(1, 129, 1000, 6), "0", 1, 16),
    (_c(1, 130, 2047, 6), None, 2, 16),
    (_c(1, 77, 4096, 6), None, 4, 16),
]
# ---- the safety net (OG_SINKHORN_FORCE_TIMEOUT=1): one to four columns per thread, more rows than the 16 waves ----
FALLBACK = [_c(2, 1, 1, 2), _c(1, 40, 1025, 3), _c(1, 40, 2049, 3), _c(1, 33, 4096, 3), _c(1, 300, 3000, 2)]

# ---- the raw ABI on the streaming schedule: case, (OG_SK_FAST_ROWS, OG_SK_FAST_NT) ----
RAW = [(_c(2, 37, 53, 5), None), (_c(1, 70, 2501, 5), None), (_c(1, 70, 2501, 5), (128, 1))]

# ---- ragged streaming: widest pair first, then smaller ones with a (1, 1) pair and one with m < 32 -> the geometry class of n_max ----
RAGGED = {
    200: [(150, 200), (1, 1), (20, 90), (64, 33)],
    600: [(100, 600), (1, 1), (20, 300), (70, 513)],
    1100: [(70, 1100), (1, 1), (20, 700), (40, 1025)],
    2100: [(40, 2100), (1, 1), (20, 1500), (33, 2049)],
}
RAGGED_ITERS = 6


def ordinary_cases():
    seen = []
    for c in PLAIN + FORCED + [NARROW_IGNORES_OVERRIDES] + [r[0] for r in RESIDENT] + FALLBACK + [r[0] for r in RAW]:
        if c not in seen:
            seen.append(c)
    return seen
