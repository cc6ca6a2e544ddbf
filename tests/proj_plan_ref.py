"""The routing of the q | k | v projections and of the message MLP, restated in Python for the tests that assert which kernels ran
(tests/test_gpu_proj_mlp_forms.py) and for the check of csrc/og_proj_plan.h on the CPU (tests/test_proj_plan_cpu.py).

Written from the call sites as they stood BEFORE the plan header existed -- og_forward*'s lambdas (proj_small_ok / proj_stream_ok / proj_wstat_ok,
qkv_proj, the cross layer's side-0 branch), og_proj_block, og_proj_small_wanted / og_proj_stream_wanted / og_proj_wstat_wanted and
og_gemm_f16x3_row_split_ok -- and NOT from the header, so that the two can disagree.  It restates what those callers tested; what only the
launchers refused (a misaligned workspace, a matrix wider than the kernel's bias area) is outside it, and the sweeps keep to requests
og_forward* can make: planes as wide as the matrix, addresses that are multiples of 16, copies of the matrix that exist exactly where
packed_layout packs them.

A step is (family, row0, rows, split_row, a0, a1, b0, b1, relu): the launch's rows, and its column ranges in the unit of the family (32-column
blocks, 256-column slabs, 128-column groups, channels).  A GEMM step with split_row is the row-split launch: rows below it stop at column a1.
"""
from collections import Counter, namedtuple

SMALL, WSTAT, STREAM, GEMM = "small", "wstat", "stream", "gemm"
FAMILIES = (SMALL, WSTAT, STREAM, GEMM)
Knobs = namedtuple("Knobs", "proj_small proj_stream gemm_row_split gemm_tile gemm_big2", defaults=(-1, -1, 1, 0, 1))      # og_knobs.h: unset
MAX_ROWS = 1 << 30


def _cdiv(a, b):
    return (a + b - 1) // b


def small_wanted(R, kn):
    """og_proj_small_wanted"""
    return kn.proj_small != 0 if kn.proj_small >= 0 else R <= 8192


def stream_wanted(M, K, full, kn):
    """og_proj_stream_wanted"""
    if kn.proj_stream == 2:
        return M > 8192 and (K == 128 or full)
    if kn.proj_stream >= 0:
        return kn.proj_stream != 0 and M > 0
    return M > 8192 and K == 128


def gemm_row_split_ok(M, N, split_row, split_n, kn):
    """og_gemm_f16x3_row_split_ok for the launch the cross layer asks about: split-f16 planes out, one plain problem."""
    if split_row <= 0 or split_row >= M or split_row % 256 or split_n <= 0 or split_n >= N or split_n % 256 or M % 256 or N % 256:
        return False
    blocks = (split_row // 256) * (split_n // 256) + ((M - split_row) // 256) * (N // 256)
    big_tile = N >= 256 if kn.gemm_tile == 256 else (N % 256 == 0 and blocks >= 192 and kn.gemm_tile != 128)       # gemm_big_tile_allowed
    return bool(kn.gemm_row_split) and blocks >= 192 and big_tile and bool(kn.gemm_big2)


class Forward:
    """The facts of one og_forward* call its projection routing reads (api.hip: forward_impl)."""

    def __init__(self, D, T0, T1, favor=False, ragged=False, knobs=Knobs(), plane_bits=0, has_small=None, has_big=None):
        self.D, self.T0, self.T1, self.T = D, T0, T1, T0 + T1
        self.favor, self.ragged, self.kn, self.plane_bits = favor, ragged, knobs, plane_bits
        self.WQ = 2 * D if favor else D                       # qk_width, qkv_width
        self.QW = 2 * self.WQ + D
        # packed_layout: the small-batch copy at K = 256 / 128 when the width is whole 32-column blocks, the batch copy at D = 128 only
        self.has_small = (not favor and D in (256, 128) and self.QW % 32 == 0) if has_small is None else has_small
        self.has_big = (not favor and D == 128 and self.QW % 128 == 0) if has_big is None else has_big

    def small_ok(self, R):
        return self.has_small and not self.favor and small_wanted(R, self.kn) and R < MAX_ROWS

    def stream_ok(self, R, full=False):
        return (self.has_big and not self.favor and stream_wanted(R if R < MAX_ROWS else 0, self.D, full, self.kn) and R < MAX_ROWS and self.QW % 64 == 0
                and not self.plane_bits & 127)

    def wstat_ok(self, R, units):
        wanted = self.D == 256 and 8192 < R < MAX_ROWS                                  # og_proj_wstat_wanted
        return self.has_small and not self.favor and not self.ragged and wanted and self.WQ == 256 and self.QW % 8 == 0 and units >= 2048

    def rows(self, r0, R, c0, c1):
        """The lambda qkv_proj: token rows [r0, r0 + R), columns [c0, c1)."""
        QW = self.QW
        if self.small_ok(R) and c0 % 32 == 0 and c1 % 32 == 0:
            return [(SMALL, r0, R, 0, 0, 0, c0 // 32, c1 // 32, 0)]
        if c0 % 256 == 0 and c1 % 256 == 0 and self.wstat_ok(R, _cdiv(R, 32) * ((c1 - c0) // 256)):
            return [(WSTAT, r0, R, 0, 0, 0, c0 // 256, c1 // 256, 0)]
        if self.stream_ok(R, c0 == 0 and c1 == QW) and c0 % 128 == 0 and c1 % 128 == 0 and (r0 * QW * 2) % 128 == 0:
            return [(STREAM, r0, R, 0, 0, 0, c0 // 128, c1 // 128, 0)]
        cut = 2 * self.WQ if self.favor else c1               # favor_relu: the feature blocks carry the ReLU, the value block does not
        mid = cut if c0 < cut < c1 else c1
        return [(GEMM, r0, R, 0, 0, 0, x0, x1, int(self.favor and x0 < 2 * self.WQ)) for x0, x1 in ((c0, mid), (mid, c1)) if x1 > x0]

    def self_layer(self):
        return self.rows(0, self.T, 0, self.QW)

    def cross_side0(self):
        """q of image 0 + q | k | v of image 1: one launch with a row split where a kernel takes it, else image 1 first, then image 0."""
        T, T0, T1, WQ, QW = self.T, self.T0, self.T1, self.WQ, self.QW
        if self.small_ok(T) and T0 % 32 == 0 and WQ % 32 == 0:
            return [(SMALL, 0, T, T0, 0, WQ // 32, 0, QW // 32, 0)]
        if self.stream_ok(T) and T0 % 128 == 0 and WQ % 128 == 0:
            return [(STREAM, 0, T, T0, 0, WQ // 128, 0, QW // 128, 0)]
        if not self.favor and not self.ragged and T < MAX_ROWS and gemm_row_split_ok(T, QW, T0, WQ, self.kn):
            if self.wstat_ok(T, T0 // 32 + _cdiv(T1, 32) * 3):
                return [(WSTAT, 0, T, T0, 0, WQ // 256, 0, QW // 256, 0)]
            return [(GEMM, 0, T, T0, 0, WQ, 0, QW, 0)]
        return self.rows(T0, T1, 0, QW) + self.rows(0, T0, 0, WQ)

    def cross_kv(self):
        """k | v of the updated image 0"""
        return self.rows(0, self.T0, self.WQ, self.QW)

    def stage(self):
        """The three requests of a GNN stage, in launch order."""
        return [self.self_layer(), self.cross_side0(), self.cross_kv()]


def plan_stage_entry(M, K, N, a, b, ldy, split_row=0, plane_bits=0, knobs=Knobs()):
    """og_proj_block (mlp_fused.hip).  a, b: block ranges (units of 32 channels) of the rows below / from split_row.  -> one step."""
    mode = knobs.proj_stream
    split_bad = lambda tile: 0 < split_row < M and split_row % tile != 0
    if (mode < 0 and K == 256 and 8192 < M < MAX_ROWS and ldy == N and all(v % 8 == 0 for v in (*a, *b)) and ldy % 8 == 0 and not split_bad(32)
            and not plane_bits & 15):                                                        # whole slabs, planes as wide as the matrix
        return [(WSTAT, 0, M, split_row, a[0] // 8, a[1] // 8, b[0] // 8, b[1] // 8, 0)]
    if ((mode != 0 if mode >= 0 else M > 8192) and N % 128 == 0                              # more than 8192 rows, a batch stream exists
            and all(v % 4 == 0 for v in (*a, *b)) and a[1] - a[0] <= 32 and b[1] - b[0] <= 32    # whole 128-channel groups, at most 8 of them
            and ldy % 64 == 0 and not split_bad(128)                                         # plane rows of whole lines, a tile-aligned split
            and not plane_bits & 127):                                                       # 128-byte aligned planes
        return [(STREAM, 0, M, split_row, a[0] // 4, a[1] // 4, b[0] // 4, b[1] // 4, 0)]
    return [(SMALL, 0, M, split_row, *a, *b, 0)]


def kernel_of(step, K):
    """The instance a step launches in the default environment.  A GEMM step: og_launch_gemm_f16x3's rule (tests/test_gpu_gemm_forms.py restates it)."""
    family, _, rows, split_row, a0, a1, b0, b1, relu = step
    if family == SMALL:
        return f"proj_small_kernel<{K}>"
    if family == STREAM:
        return f"proj_stream_kernel<{K}>"
    if family == WSTAT:
        return "proj_wstat_kernel"
    from tests.test_gpu_gemm_forms import expected_f16x3
    return expected_f16x3(rows, b1 - b0, K, planes=True, relu=bool(relu))


def expected_mlp(M, D, b0_aligned=True, b3_aligned=True):
    """og_launch_mlp_fused (mlp_fused.hip): 32-token workgroups up to 8192 rows (og_mlp_small_wanted) when both
    biases can be read as 16-byte vectors, the 128-token tile kernel otherwise."""
    small = M <= 8192 and b0_aligned and b3_aligned
    return f"mlp_small_kernel<{D}>" if small else f"mlp_fused_kernel<{D}>"


def expected_proj_block(M, K, N, a, b, ldy, split_row=0, planes_aligned=True, plane_bits=None):
    """og_proj_block -> the kernel it launches.  planes_aligned=False: planes at a multiple of 64 bytes that is not one of 128."""
    bits = (0 if planes_aligned else 64) if plane_bits is None else plane_bits
    return kernel_of(plan_stage_entry(M, K, N, a, b, ldy, split_row, bits)[0], K)


def forward_sequence(D, B, m, n, stages=1, favor=False, lens=None):
    """One og_forward* call's projection and message-MLP launches in launch order, over `stages` self + cross layers (the packed biases start
    256-byte aligned sections: both aligned).  lens: ([m_b], [n_b]) of a ragged batch."""
    T0, T1 = (sum(lens[0]), sum(lens[1])) if lens else (B * m, B * n)
    f = Forward(D, T0, T1, favor=favor, ragged=lens is not None)
    names = lambda steps: [kernel_of(s, D) for s in steps]
    one = (names(f.self_layer()) + [expected_mlp(T0 + T1, D)]                 # self layer: both images in one launch each
           + names(f.cross_side0()) + [expected_mlp(T0, D)]                   # side 0
           + names(f.cross_kv()) + [expected_mlp(T1, D)])                     # k | v of the updated image 0, side 1
    return one * stages


def expected_forward(D, B, m, n, stages=1):
    """The multiset of the four kernels of mlp_fused.hip in forward_sequence (what the first version of this restatement counted)."""
    four = ("mlp_small_kernel<", "mlp_fused_kernel<", "proj_small_kernel<", "proj_stream_kernel<")
    return Counter(k for k in forward_sequence(D, B, m, n, stages) if k.startswith(four))
