// The two training-step pieces either side of the matcher (reference models/matching_module.py:83-105):
//
//  * og_gt_matches -- models/gt_matches_generation.py `generate_gt_matches`: reproject the keypoints both ways
//    (utils/misc.py:21-103), nearest neighbour in the other image both ways, mutual check, labels
//    matched (j) / unmatched (-1) / ignore (-2).  Three kernels, no B x M x N buffer:
//      reproject_kernel  one thread per keypoint and direction; 3x3 inverses by the adjugate, all in fp64
//      nn_kernel         all-pairs nearest neighbour: a workgroup holds 64 queries (one per lane), its 4 waves split every
//                        LDS chunk of float2 targets between them; exact dx*dx + dy*dy in fp64, strict < (lowest index on ties)
//      label_kernel      mutual check, validity masks and -- apply_thresholds only -- the distance rules
//    Everything between the fp32 inputs and the labels is fp64 with contraction off, in a fixed operation order, so that
//    tests/supervision_ref.py (the same statements as float64 torch ops) reproduces every label bit for bit.
//
//  * og_criterion_forward / _backward -- utils/losses.py `criterion`: the NLL over `scores` (dustbins included) and, with
//    a margin, the triplet / hinge metric loss on the cosine distance of the context descriptors:
//      norm_kernel       1 / max(|x|, 1e-12) per keypoint (F.normalize), on the channel-first [B][D][n] tensors as they lie
//      gram_kernel       cos = a.b on exact-fp32 MFMA (v_mfma_f32_32x32x2_f32), dist = 0.25 (|a^|^2 + |b^|^2) - 0.5 cos, which is
//                        0.5 (1 - cos) bit for bit unless a descriptor is all zero (a^ = 0: utils/misc.py's
//                        0.25 |a^ - b^|^2 is then 0.25, not 0.5); the epilogue does the
//                        four argmins (row / column, over dist and over dist with the positives gt0[i] == j at +inf) and
//                        merges them across workgroups with packed 64-bit atomicMin on (orderable value, index)
//      pair_loss_kernel  one workgroup per pair: the per-pair means of the NLL and of the hinge terms, fixed-order sums; a
//                        masked minimum of +inf (the positive is the only entry of its row / column) gives the term
//                        `margin`, as the reference's argmin of an all-inf line does (it gathers d_an = d_ap)
//      finish_kernel     the sums over pairs in pair order, / B  -> loss, metric_loss (bit-identical from run to run)
//    backward: nll_grad_kernel writes the dense grad_scores the Sinkhorn backward takes; metric_scatter_kernel adds
//    0.5 c (a^ - b^) for the O(M + N) distance entries that carry a gradient (float atomics: one row can be the hardest
//    negative of many anchors); normalize_grad_kernel applies the Jacobian of the normalisation in place.
#include "og_block.h"

namespace {

constexpr float kEpsNorm = 1e-12f;     // F.normalize
constexpr double kEpsW = 1e-8;         // perspective_transform / reproject_3d: divide by w + eps

__device__ __forceinline__ unsigned int sv_orderable(float v) {
    const unsigned int b = __float_as_uint(v);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float sv_unorderable(unsigned int k) {
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k);
}
__device__ __forceinline__ unsigned long long sv_key(float v, int idx) {
    return ((unsigned long long)sv_orderable(v) << 32) | (unsigned)idx;
}

// ------------------------------------------------------------------------------------------------ ground-truth matches
struct GtWs {
    double2* proj0;   // [B][m] keypoints0 mapped into image 1
    double2* proj1;   // [B][n] keypoints1 mapped into image 0
    double* d2_0;     // [B][m] squared distance to the nearest keypoint1
    double* d2_1;     // [B][n]
    int* nn0;         // [B][m]
    int* nn1;         // [B][n]
    int* valid0;      // [B][m] depth known
    int* valid1;      // [B][n]
};

static GtWs gt_layout(void* ws, int B, int m, int n) {
    GtWs w{};
    char* p = (char*)ws;
    auto take = [&](size_t bytes) { char* r = p; p += og_round_up((int64_t)bytes, 256); return r; };
    w.proj0 = (double2*)take(sizeof(double2) * (size_t)B * m);
    w.proj1 = (double2*)take(sizeof(double2) * (size_t)B * n);
    w.d2_0 = (double*)take(sizeof(double) * (size_t)B * m);
    w.d2_1 = (double*)take(sizeof(double) * (size_t)B * n);
    w.nn0 = (int*)take(sizeof(int) * (size_t)B * m);
    w.nn1 = (int*)take(sizeof(int) * (size_t)B * n);
    w.valid0 = (int*)take(sizeof(int) * (size_t)B * m);
    w.valid1 = (int*)take(sizeof(int) * (size_t)B * n);
    return w;
}

static size_t gt_bytes(int B, int m, int n) {
    const int64_t pm = (int64_t)B * m, pn = (int64_t)B * n;
    return og_round_up(16 * pm, 256) + og_round_up(16 * pn, 256) + og_round_up(8 * pm, 256) + og_round_up(8 * pn, 256) +
           2 * og_round_up(4 * pm, 256) + 2 * og_round_up(4 * pn, 256);
}

struct GtArgs {
    int B, m, n;
    const float* kpts0; const float* kpts1;   // [B][m][2], [B][n][2]
    int type;                                 // 0 perspective, 1 3d_reprojection
    const float* H;                           // [B][3][3]
    const float* K0; const float* K1; const float* R; const float* T;
    const float* depth0; int dh0, dw0;        // dh0 == 0: per keypoint [B][m]; else a map [B][dh0][dw0]
    const float* depth1; int dh1, dw1;
};

// inverse of the row-major 3x3 matrix a (fp32) by the adjugate, in fp64
__device__ void inv3(const float* a_, double* o) {
#pragma clang fp contract(off)  // fixed rounding: tests/supervision_ref.py restates these statements
    double a[9];
    for (int e = 0; e < 9; ++e) a[e] = (double)a_[e];
    const double c00 = a[4] * a[8] - a[5] * a[7];
    const double c01 = a[5] * a[6] - a[3] * a[8];
    const double c02 = a[3] * a[7] - a[4] * a[6];
    const double det = a[0] * c00 + a[1] * c01 + a[2] * c02;
    o[0] = c00 / det;
    o[1] = (a[2] * a[7] - a[1] * a[8]) / det;
    o[2] = (a[1] * a[5] - a[2] * a[4]) / det;
    o[3] = c01 / det;
    o[4] = (a[0] * a[8] - a[2] * a[6]) / det;
    o[5] = (a[2] * a[3] - a[0] * a[5]) / det;
    o[6] = c02 / det;
    o[7] = (a[1] * a[6] - a[0] * a[7]) / det;
    o[8] = (a[0] * a[4] - a[1] * a[3]) / det;
}

// y = A [x0, x1, x2]  (row r: (A_r0 x0 + A_r1 x1) + A_r2 x2)
__device__ __forceinline__ void mv3(const double* A, double x0, double x1, double x2, double* y) {
#pragma clang fp contract(off)  // fixed rounding: tests/supervision_ref.py restates these statements
    for (int r = 0; r < 3; ++r) y[r] = A[3 * r] * x0 + A[3 * r + 1] * x1 + A[3 * r + 2] * x2;
}

// torch indexing of one depth-map axis: i in [-size, size) (negative wraps), else out of range
__device__ __forceinline__ bool wrap_index(float x, int size, int& out) {
    if (!(fabsf(x) < 9.0e18f)) return false;
    const long long i = (long long)x;                     // .type(torch.int64): truncation toward zero
    if (i < -(long long)size || i >= (long long)size) return false;
    out = (int)(i < 0 ? i + size : i);
    return true;
}

// grid (ceil(max(m, n) / 256), B, 2): z = 0 maps keypoints0 into image 1 with the transformation, z = 1 keypoints1 into image 0
// with its inverse (get_inverse_transformation: K0 <-> K1, R^T, -R^T T, depth1)
__global__ __launch_bounds__(256) void reproject_kernel(GtArgs a, GtWs w, int* __restrict__ status) {
#pragma clang fp contract(off)  // fixed rounding: tests/supervision_ref.py restates these statements
    const int b = blockIdx.y, dir = blockIdx.z;
    const int t = blockIdx.x * 256 + threadIdx.x;
    const int cnt = dir ? a.n : a.m;
    if (t >= cnt) return;
    const float* kp = (dir ? a.kpts1 : a.kpts0) + ((int64_t)b * cnt + t) * 2;
    const double x = (double)kp[0], y = (double)kp[1];
    double q[3];
    int valid = 1;
    if (a.type == 0) {
        double Hm[9];
        if (dir) inv3(a.H + 9 * b, Hm);
        else for (int e = 0; e < 9; ++e) Hm[e] = (double)a.H[9 * b + e];
        mv3(Hm, x, y, 1.0, q);
    } else {
        const float* Ka = (dir ? a.K1 : a.K0) + 9 * b;
        const float* Kb = (dir ? a.K0 : a.K1) + 9 * b;
        const float* Rm = a.R + 9 * b;
        const float* Tv = a.T + 3 * b;
        double Ki[9], Rd[9], Kd[9], Td[3];
        inv3(Ka, Ki);
        for (int e = 0; e < 9; ++e) Kd[e] = (double)Kb[e];
        if (dir) {
            for (int r = 0; r < 3; ++r)
                for (int c = 0; c < 3; ++c) Rd[3 * r + c] = (double)Rm[3 * c + r];
            for (int r = 0; r < 3; ++r) Td[r] = -(Rd[3 * r] * (double)Tv[0] + Rd[3 * r + 1] * (double)Tv[1] + Rd[3 * r + 2] * (double)Tv[2]);
        } else {
            for (int e = 0; e < 9; ++e) Rd[e] = (double)Rm[e];
            for (int r = 0; r < 3; ++r) Td[r] = (double)Tv[r];
        }
        const float* dp = dir ? a.depth1 : a.depth0;
        const int dh = dir ? a.dh1 : a.dh0, dw = dir ? a.dw1 : a.dw0;
        float dv = 0.f;
        if (dh == 0) {
            dv = dp[(int64_t)b * cnt + t];
        } else {
            int iy, ix;
            if (wrap_index(kp[1], dh, iy) && wrap_index(kp[0], dw, ix)) dv = dp[((int64_t)b * dh + iy) * dw + ix];
            else atomicOr(status, 1 << dir);               // the reference raises IndexError here; nothing is read
        }
        valid = !(fabsf(dv) <= 1e-8f);                      // ~torch.isclose(depth, 0): |depth| <= atol
        double p[3], r3[3];
        mv3(Ki, x, y, 1.0, p);
        const double d = (double)dv;
        p[0] = p[0] * d; p[1] = p[1] * d; p[2] = p[2] * d;
        mv3(Rd, p[0], p[1], p[2], r3);
        r3[0] = r3[0] + Td[0]; r3[1] = r3[1] + Td[1]; r3[2] = r3[2] + Td[2];
        mv3(Kd, r3[0], r3[1], r3[2], q);
    }
    const double wz = q[2] + kEpsW;
    (dir ? w.proj1 : w.proj0)[(int64_t)b * cnt + t] = make_double2(q[0] / wz, q[1] / wz);
    (dir ? w.valid1 : w.valid0)[(int64_t)b * cnt + t] = valid;
}

constexpr int NN_Q = 64;          // queries per workgroup (one per lane of each wave)
constexpr int NN_CHUNK = 1024;    // targets per LDS chunk (8 KB of float2); wave w scans [w * 256, (w + 1) * 256)

// grid (ceil(max(m, n) / 64), B, 2): z = 0 queries proj0 against keypoints1, z = 1 proj1 against keypoints0
__global__ __launch_bounds__(256) void nn_kernel(GtArgs a, GtWs w) {
#pragma clang fp contract(off)  // fixed rounding: tests/supervision_ref.py restates these statements
    __shared__ float2 tgt[NN_CHUNK];
    __shared__ double bd[4][NN_Q];
    __shared__ int bj[4][NN_Q];
    const int b = blockIdx.y, dir = blockIdx.z;
    const int nq = dir ? a.n : a.m, nt = dir ? a.m : a.n;
    const int q0 = blockIdx.x * NN_Q;
    if (q0 >= nq) return;                                  // uniform across the workgroup
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int qi = q0 + lane;
    double2 q = make_double2(0.0, 0.0);
    if (qi < nq) q = (dir ? w.proj1 : w.proj0)[(int64_t)b * nq + qi];
    const float2* T = reinterpret_cast<const float2*>(dir ? a.kpts0 : a.kpts1) + (int64_t)b * nt;
    double best = __builtin_huge_val();
    int bi = -1;
    for (int c0 = 0; c0 < nt; c0 += NN_CHUNK) {
        const int len = min(NN_CHUNK, nt - c0);
        for (int e = threadIdx.x; e < len; e += 256) tgt[e] = T[c0 + e];
        __syncthreads();
        const int lo = wave * (NN_CHUNK / 4), hi = min(lo + NN_CHUNK / 4, len);
        for (int e = lo; e < hi; ++e) {
            const float2 p = tgt[e];
            const double dx = q.x - (double)p.x;
            const double dy = q.y - (double)p.y;
            const double d2 = dx * dx + dy * dy;
            if (d2 < best || bi < 0) { best = d2; bi = c0 + e; }   // ascending index: strict < keeps the first minimum
        }
        __syncthreads();
    }
    bd[wave][lane] = best;
    bj[wave][lane] = bi;
    __syncthreads();
    if (wave == 0 && qi < nq) {
        for (int v = 1; v < 4; ++v) {
            const int j = bj[v][lane];
            if (j < 0) continue;
            const double d = bd[v][lane];
            if (bi < 0 || d < best || (d == best && j < bi)) { best = d; bi = j; }
        }
        (dir ? w.d2_1 : w.d2_0)[(int64_t)b * nq + qi] = best;
        (dir ? w.nn1 : w.nn0)[(int64_t)b * nq + qi] = bi;
    }
}

// grid (ceil(max(m, n) / 256), B, 2): labels of image 0 (z = 0) / image 1 (z = 1)
__global__ __launch_bounds__(256) void label_kernel(int B, int m, int n, GtWs w, int apply_thresholds, double pos, double neg,
                                                    int64_t* __restrict__ gt0, int64_t* __restrict__ gt1) {
#pragma clang fp contract(off)
    const int b = blockIdx.y, dir = blockIdx.z;
    const int t = blockIdx.x * 256 + threadIdx.x;
    const int cnt = dir ? n : m, oth = dir ? m : n;
    if (t >= cnt) return;
    const int* nnS = (dir ? w.nn1 : w.nn0) + (int64_t)b * cnt;
    const int* nnO = (dir ? w.nn0 : w.nn1) + (int64_t)b * oth;
    const double* dS = (dir ? w.d2_1 : w.d2_0) + (int64_t)b * cnt;
    const double* dO = (dir ? w.d2_0 : w.d2_1) + (int64_t)b * oth;
    const int* vS = (dir ? w.valid1 : w.valid0) + (int64_t)b * cnt;
    const int* vO = (dir ? w.valid0 : w.valid1) + (int64_t)b * oth;
    const int j = nnS[t];
    const bool mutual = nnO[j] == t;
    int64_t v = mutual ? (int64_t)j : -1;
    if (apply_thresholds) {                  // gt_matches_generation.py:59-79 as in-place writes, in source order
        if (mutual) {
            const double sym = 0.5 * (sqrt(dS[t]) + sqrt(dO[j]));
            if (sym > pos) v = -2;
            if (sym > neg) v = -1;
        } else if (sqrt(dS[t]) <= neg) {
            v = -2;
        }
    }
    if (!vS[t]) v = -2;
    if (apply_thresholds && mutual && !vO[j]) v = -2;
    (dir ? gt1 : gt0)[(int64_t)b * cnt + t] = v;
}

// ------------------------------------------------------------------------------------------------ criterion
struct CritWs {
    float* pair;                  // [B][2] per-pair NLL / metric terms
    int* counts;                  // [B][3] matched, unmatched0, unmatched1
    float* inv0;                  // [B][m] 1 / max(|a_i|, eps)
    float* inv1;                  // [B][n]
    float* dap;                   // [B][m] dist(i, gt0[i])
    unsigned long long* row;      // [B][m] argmin_j dist(i, j)
    unsigned long long* rowm;     // [B][m] the same with the positives at +inf
    unsigned long long* col;      // [B][n] argmin_i dist(i, j)
    unsigned long long* colm;     // [B][n]
};

static CritWs crit_layout(void* ws, int B, int m, int n, bool margin) {
    CritWs w{};
    char* p = (char*)ws;
    auto take = [&](size_t bytes) { char* r = p; p += og_round_up((int64_t)bytes, 256); return r; };
    w.pair = (float*)take(sizeof(float) * 2 * (size_t)B);
    w.counts = (int*)take(sizeof(int) * 3 * (size_t)B);
    if (margin) {
        w.row = (unsigned long long*)take(8 * (size_t)B * m);
        w.rowm = (unsigned long long*)take(8 * (size_t)B * m);
        w.col = (unsigned long long*)take(8 * (size_t)B * n);
        w.colm = (unsigned long long*)take(8 * (size_t)B * n);
        w.inv0 = (float*)take(sizeof(float) * (size_t)B * m);
        w.inv1 = (float*)take(sizeof(float) * (size_t)B * n);
        w.dap = (float*)take(sizeof(float) * (size_t)B * m);
    }
    return w;
}

static size_t crit_bytes(int B, int m, int n, bool margin) {
    size_t s = og_round_up(8 * (int64_t)B, 256) + og_round_up(12 * (int64_t)B, 256);
    if (margin) s += 2 * og_round_up(8 * (int64_t)B * m, 256) + 2 * og_round_up(8 * (int64_t)B * n, 256) +
                     2 * og_round_up(4 * (int64_t)B * m, 256) + og_round_up(4 * (int64_t)B * n, 256);
    return s;
}

// grid (ceil(cnt / 256), B, 2): thread = one keypoint of image z, sums its D channels (coalesced across threads)
__global__ __launch_bounds__(256) void norm_kernel(const float* __restrict__ d0, const float* __restrict__ d1, int m, int n, int D,
                                                   float* __restrict__ inv0, float* __restrict__ inv1) {
    const int b = blockIdx.y, dir = blockIdx.z;
    const int cnt = dir ? n : m;
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= cnt) return;
    const float* x = (dir ? d1 : d0) + (int64_t)b * D * cnt + t;
    float s = 0.f;
    for (int k = 0; k < D; ++k) { const float v = x[(int64_t)k * cnt]; s = fmaf(v, v, s); }
    (dir ? inv1 : inv0)[(int64_t)b * cnt + t] = 1.f / fmaxf(sqrtf(s), kEpsNorm);
}

constexpr int GT = 64;            // Gram tile: 64 x 64, 4 waves as 2 x 2, each one 32 x 32 MFMA tile
constexpr int GK = 32;            // k slab
constexpr int GLD = GT + 4;       // k-major LDS row (floats)

// grid (ceil(n / 64), ceil(m / 64), B).  Operands are the channel-first [D][cnt] descriptors: k-major as they lie.
__global__ __launch_bounds__(256) void gram_kernel(const float* __restrict__ d0, const float* __restrict__ d1, const int64_t* __restrict__ gt0,
                                                   int m, int n, int D, CritWs w) {
    __shared__ __attribute__((aligned(16))) float As[GK * GLD];
    __shared__ __attribute__((aligned(16))) float Bs[GK * GLD];
    __shared__ float sinv0[GT], sinv1[GT];
    __shared__ float sq0[GT], sq1[GT];                    // 0.25 |x^|^2: 0.25, or 0 for an all-zero descriptor (F.normalize's clamp)
    __shared__ int spos[GT];
    const int b = blockIdx.z;
    const int m0 = blockIdx.y * GT, n0 = blockIdx.x * GT;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const float* A = d0 + (int64_t)b * D * m;
    const float* Bm = d1 + (int64_t)b * D * n;
    if (tid < GT) {
        const int i = m0 + tid;
        sinv0[tid] = i < m ? w.inv0[(int64_t)b * m + i] : 0.f;
        sq0[tid] = sinv0[tid] == 1.f / kEpsNorm ? 0.f : 0.25f;
        const int64_t g = i < m ? gt0[(int64_t)b * m + i] : -1;
        spos[tid] = (g >= 0 && g < n) ? (int)g : -1;
    } else if (tid < 2 * GT) {
        const int j = n0 + tid - GT;
        sinv1[tid - GT] = j < n ? w.inv1[(int64_t)b * n + j] : 0.f;
        sq1[tid - GT] = sinv1[tid - GT] == 1.f / kEpsNorm ? 0.f : 0.25f;
    }
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    const int sc = tid & 63, sk = tid >> 6;               // staging: column sc, k rows sk, sk + 4, ...
    for (int k0 = 0; k0 < D; k0 += GK) {
#pragma unroll
        for (int p = 0; p < GK / 4; ++p) {
            const int k = k0 + sk + 4 * p;
            const int i = m0 + sc, j = n0 + sc;
            As[(sk + 4 * p) * GLD + sc] = (k < D && i < m) ? A[(int64_t)k * m + i] : 0.f;
            Bs[(sk + 4 * p) * GLD + sc] = (k < D && j < n) ? Bm[(int64_t)k * n + j] : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < GK; kk += 2) {
            const float a = As[(kk + (lane >> 5)) * GLD + wm * 32 + (lane & 31)];
            const float bv = Bs[(kk + (lane >> 5)) * GLD + wn * 32 + (lane & 31)];
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, bv, acc, 0, 0, 0);
        }
        __syncthreads();
    }
    // ---- epilogue: dist, the four argmins, d_ap ----
    const int cl = wn * 32 + (lane & 31);
    const int j = n0 + cl;
    const bool jok = j < n;
    const unsigned long long NONE = ~0ull;
    unsigned long long cbest = NONE, cbestm = NONE;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int rl = wm * 32 + mfma32_row(r, lane);
        const int i = m0 + rl;
        const bool ok = jok && i < m;
        // one rounding of 0.5 - 0.5 (acc inv0) inv1, spelled out so that it does not hang on the compiler's contraction
        const float d = fmaf(-0.5f * (acc[r] * sinv0[rl]), sinv1[cl], sq0[rl] + sq1[cl]);
        const bool positive = spos[rl] == j;
        if (ok && positive) w.dap[(int64_t)b * m + i] = d;
        const float dm = positive ? __builtin_huge_valf() : d;
        unsigned long long kr = ok ? sv_key(d, j) : NONE, krm = ok ? sv_key(dm, j) : NONE;
        const unsigned long long kc = ok ? sv_key(d, i) : NONE, kcm = ok ? sv_key(dm, i) : NONE;
        cbest = kc < cbest ? kc : cbest;
        cbestm = kcm < cbestm ? kcm : cbestm;
        // row i: min over the 32 lanes of this half-wave (they hold the 32 columns)
#pragma unroll
        for (int o = 16; o > 0; o >>= 1) {
            const unsigned long long x = __shfl_xor(kr, o, 64), xm = __shfl_xor(krm, o, 64);
            kr = x < kr ? x : kr;
            krm = xm < krm ? xm : krm;
        }
        if ((lane & 31) == 0 && i < m && kr != NONE) {
            atomicMin(w.row + (int64_t)b * m + i, kr);
            atomicMin(w.rowm + (int64_t)b * m + i, krm);
        }
    }
    {   // column j: the two half-waves hold rows 0-3, 8-11, ... and 4-7, 12-15, ...
        const unsigned long long x = __shfl_xor(cbest, 32, 64), xm = __shfl_xor(cbestm, 32, 64);
        cbest = x < cbest ? x : cbest;
        cbestm = xm < cbestm ? xm : cbestm;
        if (lane < 32 && cbest != NONE) {
            atomicMin(w.col + (int64_t)b * n + j, cbest);
            atomicMin(w.colm + (int64_t)b * n + j, cbestm);
        }
    }
}

// grid (B): per-pair terms of utils/losses.py -- every sum in a fixed order (thread-strided, then block_sum of og_block.h)
__global__ __launch_bounds__(256) void pair_loss_kernel(const float* __restrict__ scores, const int64_t* __restrict__ gt0,
                                                        const int64_t* __restrict__ gt1, int m, int n, int margin_on, float margin, CritWs w) {
    __shared__ float red[4];
    __shared__ int ired[4];
    const int b = blockIdx.x;
    const float* S = scores + (int64_t)b * (m + 1) * (n + 1);
    const int64_t* g0 = gt0 + (int64_t)b * m;
    const int64_t* g1 = gt1 + (int64_t)b * n;
    int cm = 0, c0 = 0, c1 = 0;
    float sm = 0.f, s0 = 0.f, s1 = 0.f, hm = 0.f, h0 = 0.f, h1 = 0.f;
    for (int i = threadIdx.x; i < m; i += 256) {
        const int64_t g = g0[i];
        if (g >= 0 && g < n) {
            ++cm;
            sm -= S[(int64_t)i * (n + 1) + g];
            if (margin_on) {
                const float dap = w.dap[(int64_t)b * m + i];
                const float an0 = sv_unorderable((unsigned)(w.rowm[(int64_t)b * m + i] >> 32));
                const float an1 = sv_unorderable((unsigned)(w.colm[(int64_t)b * n + g] >> 32));
                // +inf: no other candidate in that row / column; the backward leaves such a term without gradient
                // (select the argument, then one fmaxf: with fmaxf in both arms of the select, ROCm 7.2's gfx950 instruction selection crashes)
                const float inf = __builtin_huge_valf();
                const float t0 = an0 == inf ? margin : dap - an0 + margin, t1 = an1 == inf ? margin : dap - an1 + margin;
                hm += fmaxf(t0, 0.f) + fmaxf(t1, 0.f);
            }
        } else if (g == -1) {
            ++c0;
            s0 -= S[(int64_t)i * (n + 1) + n];
            if (margin_on) h0 += fmaxf(margin - sv_unorderable((unsigned)(w.row[(int64_t)b * m + i] >> 32)), 0.f);
        }
    }
    for (int j = threadIdx.x; j < n; j += 256) {
        if (g1[j] == -1) {
            ++c1;
            s1 -= S[(int64_t)m * (n + 1) + j];
            if (margin_on) h1 += fmaxf(margin - sv_unorderable((unsigned)(w.col[(int64_t)b * n + j] >> 32)), 0.f);
        }
    }
    cm = block_sum(cm, ired); c0 = block_sum(c0, ired); c1 = block_sum(c1, ired);
    sm = block_sum(sm, red); s0 = block_sum(s0, red); s1 = block_sum(s1, red);
    hm = block_sum(hm, red); h0 = block_sum(h0, red); h1 = block_sum(h1, red);
    if (threadIdx.x == 0) {
        // an empty set contributes 0 (torch.unique_consecutive gives it no weight)
        const float lm = cm ? sm / cm : 0.f, l0 = c0 ? s0 / c0 : 0.f, l1 = c1 ? s1 / c1 : 0.f;
        w.pair[2 * b] = lm + 0.5f * (l0 + l1);
        w.pair[2 * b + 1] = (cm ? hm / cm : 0.f) + (c0 ? h0 / c0 : 0.f) + (c1 ? h1 / c1 : 0.f);
        w.counts[3 * b] = cm; w.counts[3 * b + 1] = c0; w.counts[3 * b + 2] = c1;
    }
}

__global__ void finish_kernel(int B, CritWs w, float* __restrict__ out) {
    if (threadIdx.x != 0) return;
    float l = 0.f, mt = 0.f;
    for (int b = 0; b < B; ++b) { l += w.pair[2 * b]; mt += w.pair[2 * b + 1]; }
    out[0] = l / B;
    out[1] = mt / B;
}

// grid (ceil(max(m, n) / 256), B): the NLL's gradient entries; grad_scores is zero elsewhere (memset by the caller)
__global__ __launch_bounds__(256) void nll_grad_kernel(const int64_t* __restrict__ gt0, const int64_t* __restrict__ gt1, int B, int m, int n,
                                                       const float* __restrict__ gout, CritWs w, float* __restrict__ G) {
    const int b = blockIdx.y;
    const int t = blockIdx.x * 256 + threadIdx.x;
    const float go = gout ? gout[0] : 1.f;
    const int cm = w.counts[3 * b], c0 = w.counts[3 * b + 1], c1 = w.counts[3 * b + 2];
    float* Gb = G + (int64_t)b * (m + 1) * (n + 1);
    if (t < m) {
        const int64_t g = gt0[(int64_t)b * m + t];
        if (g >= 0 && g < n) Gb[(int64_t)t * (n + 1) + g] = -go / ((float)cm * B);
        else if (g == -1) Gb[(int64_t)t * (n + 1) + n] = -0.5f * go / ((float)c0 * B);
    }
    if (t < n && gt1[(int64_t)b * n + t] == -1) Gb[(int64_t)m * (n + 1) + t] = -0.5f * go / ((float)c1 * B);
}

// d dist(i, j) = 0.5 (a^_i - b^_j) . d a^_i  (and the mirror for b^_j): c times that, into the a^ / b^ gradient accumulators
__device__ __forceinline__ void scatter_term(const float* A, const float* Bm, float ia, float ib, int i, int j, int m, int n, int D,
                                             float c, float* gA, float* gB, int lane) {
    for (int k = lane; k < D; k += 64) {
        const float a = A[(int64_t)k * m + i] * ia, bb = Bm[(int64_t)k * n + j] * ib;
        const float g = 0.5f * c * (a - bb);
        atomicAdd(gA + (int64_t)k * m + i, g);
        atomicAdd(gB + (int64_t)k * n + j, -g);
    }
}

// grid (ceil(max(m, n) / 4), B): one wave per anchor keypoint t (image 0 and, unmatched, image 1)
__global__ __launch_bounds__(256) void metric_scatter_kernel(const float* __restrict__ d0, const float* __restrict__ d1,
                                                             const int64_t* __restrict__ gt0, const int64_t* __restrict__ gt1,
                                                             int B, int m, int n, int D, float margin, const float* __restrict__ gout,
                                                             CritWs w, float* gA0, float* gB0) {
    const int b = blockIdx.y;
    const int t = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    const float go = gout ? gout[1] : 1.f;
    const int cm = w.counts[3 * b], c0 = w.counts[3 * b + 1], c1 = w.counts[3 * b + 2];
    const float* A = d0 + (int64_t)b * D * m;
    const float* Bm = d1 + (int64_t)b * D * n;
    float* gA = gA0 + (int64_t)b * D * m;
    float* gB = gB0 + (int64_t)b * D * n;
    const float* iv0 = w.inv0 + (int64_t)b * m;
    const float* iv1 = w.inv1 + (int64_t)b * n;
    if (t < m) {
        const int64_t g = gt0[(int64_t)b * m + t];
        if (g >= 0 && g < n) {
            const int j = (int)g;
            const float wt = go / ((float)cm * B);
            const float dap = w.dap[(int64_t)b * m + t];
            const unsigned long long kr = w.rowm[(int64_t)b * m + t], kc = w.colm[(int64_t)b * n + j];
            const int jn = (int)(kr & 0xFFFFFFFFull), in = (int)(kc & 0xFFFFFFFFull);
            float cp = 0.f;
            if (dap - sv_unorderable((unsigned)(kr >> 32)) + margin > 0.f) {
                cp += wt;
                scatter_term(A, Bm, iv0[t], iv1[jn], t, jn, m, n, D, -wt, gA, gB, lane);
            }
            if (dap - sv_unorderable((unsigned)(kc >> 32)) + margin > 0.f) {
                cp += wt;
                scatter_term(A, Bm, iv0[in], iv1[j], in, j, m, n, D, -wt, gA, gB, lane);
            }
            if (cp != 0.f) scatter_term(A, Bm, iv0[t], iv1[j], t, j, m, n, D, cp, gA, gB, lane);
        } else if (g == -1) {
            const unsigned long long kr = w.row[(int64_t)b * m + t];
            if (margin - sv_unorderable((unsigned)(kr >> 32)) > 0.f) {
                const int jn = (int)(kr & 0xFFFFFFFFull);
                scatter_term(A, Bm, iv0[t], iv1[jn], t, jn, m, n, D, -go / ((float)c0 * B), gA, gB, lane);
            }
        }
    }
    if (t < n && gt1[(int64_t)b * n + t] == -1) {
        const unsigned long long kc = w.col[(int64_t)b * n + t];
        if (margin - sv_unorderable((unsigned)(kc >> 32)) > 0.f) {
            const int in = (int)(kc & 0xFFFFFFFFull);
            scatter_term(A, Bm, iv0[in], iv1[t], in, t, m, n, D, -go / ((float)c1 * B), gA, gB, lane);
        }
    }
}

// grid (ceil(cnt / 256), B, 2): g <- (g - x^ (x^ . g)) / |x|, or g / eps where |x| < eps (F.normalize's clamp), in place
__global__ __launch_bounds__(256) void normalize_grad_kernel(const float* __restrict__ d0, const float* __restrict__ d1, int m, int n, int D,
                                                             CritWs w, float* g0, float* g1) {
    const int b = blockIdx.y, dir = blockIdx.z;
    const int cnt = dir ? n : m;
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= cnt) return;
    const float* x = (dir ? d1 : d0) + (int64_t)b * D * cnt + t;
    float* g = (dir ? g1 : g0) + (int64_t)b * D * cnt + t;
    const float inv = (dir ? w.inv1 : w.inv0)[(int64_t)b * cnt + t];
    const bool clamped = inv == 1.f / kEpsNorm;
    float dot = 0.f;
    if (!clamped)
        for (int k = 0; k < D; ++k) dot = fmaf(x[(int64_t)k * cnt] * inv, g[(int64_t)k * cnt], dot);
    for (int k = 0; k < D; ++k) {
        const int64_t o = (int64_t)k * cnt;
        g[o] = (g[o] - x[o] * inv * dot) * inv;
    }
}

}  // namespace

extern "C" size_t og_gt_matches_workspace_bytes(int32_t batch, int32_t m, int32_t n) {
    if (batch <= 0 || m <= 0 || n <= 0) return 0;
    return gt_bytes(batch, m, n);
}

extern "C" int og_gt_matches(int32_t batch, int32_t m, int32_t n, const float* keypoints0, const float* keypoints1, int32_t transform,
                             const float* H, const float* K0, const float* K1, const float* R, const float* T,
                             const float* depth0, int32_t depth0_h, int32_t depth0_w, const float* depth1, int32_t depth1_h, int32_t depth1_w,
                             int32_t apply_thresholds, double positive_threshold, double negative_threshold,
                             int64_t* gt_matches0, int64_t* gt_matches1, int32_t* status_dev, void* workspace_dev, void* stream) {
    og_clear_status();
    if (batch <= 0 || m <= 0 || n <= 0 || !keypoints0 || !keypoints1 || !gt_matches0 || !gt_matches1 || !status_dev || !workspace_dev)
        return OG_E_INVALID;
    if ((uintptr_t)keypoints0 & 7 || (uintptr_t)keypoints1 & 7 || (uintptr_t)workspace_dev & 15) return OG_E_ALIGN;
    if (transform == 0) {
        if (!H) return OG_E_INVALID;
    } else if (transform == 1) {
        if (!K0 || !K1 || !R || !T || !depth0 || !depth1) return OG_E_INVALID;
        if (depth0_h < 0 || depth1_h < 0 || (depth0_h > 0 && depth0_w <= 0) || (depth1_h > 0 && depth1_w <= 0)) return OG_E_SHAPE;
    } else {
        return OG_E_FLAG;
    }
    hipStream_t st = (hipStream_t)stream;
    const GtWs w = gt_layout(workspace_dev, batch, m, n);
    GtArgs a{batch, m, n, keypoints0, keypoints1, transform, H, K0, K1, R, T, depth0, depth0_h, depth0_w, depth1, depth1_h, depth1_w};
    hipError_t e = hipMemsetAsync(status_dev, 0, sizeof(int32_t), st);
    if (e != hipSuccess) return (int)e;
    const int mx = m > n ? m : n;
    hipLaunchKernelGGL(reproject_kernel, dim3((mx + 255) / 256, batch, 2), dim3(256), 0, st, a, w, status_dev);
    hipLaunchKernelGGL(nn_kernel, dim3((mx + NN_Q - 1) / NN_Q, batch, 2), dim3(256), 0, st, a, w);
    hipLaunchKernelGGL(label_kernel, dim3((mx + 255) / 256, batch, 2), dim3(256), 0, st, batch, m, n, w, apply_thresholds,
                       positive_threshold, negative_threshold, gt_matches0, gt_matches1);
    return og_launch_status();
}

extern "C" size_t og_criterion_workspace_bytes(int32_t batch, int32_t m, int32_t n, int32_t with_margin) {
    if (batch <= 0 || m <= 0 || n <= 0) return 0;
    return crit_bytes(batch, m, n, with_margin != 0);
}

extern "C" int og_criterion_forward(const float* scores, const int64_t* gt_matches0, const int64_t* gt_matches1,
                                    const float* context_descriptors0, const float* context_descriptors1,
                                    int32_t batch, int32_t m, int32_t n, int32_t D, int32_t with_margin, float margin,
                                    float* losses, void* workspace_dev, void* stream) {
    og_clear_status();
    if (!scores || !gt_matches0 || !gt_matches1 || !losses || !workspace_dev || batch <= 0 || m <= 0 || n <= 0) return OG_E_INVALID;
    if (with_margin && (!context_descriptors0 || !context_descriptors1 || D <= 0)) return OG_E_INVALID;
    if ((uintptr_t)workspace_dev & 15) return OG_E_ALIGN;
    hipStream_t st = (hipStream_t)stream;
    const CritWs w = crit_layout(workspace_dev, batch, m, n, with_margin != 0);
    if (with_margin) {
        hipError_t e = hipMemsetAsync(w.row, 0xFF, (char*)w.inv0 - (char*)w.row, st);     // row, rowm, col, colm: "no candidate yet"
        if (e != hipSuccess) return (int)e;
        const int mx = m > n ? m : n;
        hipLaunchKernelGGL(norm_kernel, dim3((mx + 255) / 256, batch, 2), dim3(256), 0, st, context_descriptors0, context_descriptors1,
                           m, n, D, w.inv0, w.inv1);
        hipLaunchKernelGGL(gram_kernel, dim3((n + GT - 1) / GT, (m + GT - 1) / GT, batch), dim3(256), 0, st, context_descriptors0,
                           context_descriptors1, gt_matches0, m, n, D, w);
    }
    hipLaunchKernelGGL(pair_loss_kernel, dim3(batch), dim3(256), 0, st, scores, gt_matches0, gt_matches1, m, n, with_margin, margin, w);
    hipLaunchKernelGGL(finish_kernel, dim3(1), dim3(64), 0, st, batch, w, losses);
    return og_launch_status();
}

extern "C" int og_criterion_backward(const int64_t* gt_matches0, const int64_t* gt_matches1,
                                     const float* context_descriptors0, const float* context_descriptors1,
                                     int32_t batch, int32_t m, int32_t n, int32_t D, int32_t with_margin, float margin,
                                     const float* grad_losses, const void* workspace_dev, float* grad_scores,
                                     float* grad_context_descriptors0, float* grad_context_descriptors1, void* stream) {
    og_clear_status();
    if (!gt_matches0 || !gt_matches1 || !workspace_dev || batch <= 0 || m <= 0 || n <= 0) return OG_E_INVALID;
    const bool want_desc = grad_context_descriptors0 || grad_context_descriptors1;
    if (want_desc && (!with_margin || !grad_context_descriptors0 || !grad_context_descriptors1 || !context_descriptors0 ||
                      !context_descriptors1 || D <= 0))
        return OG_E_INVALID;
    if ((uintptr_t)workspace_dev & 15) return OG_E_ALIGN;
    hipStream_t st = (hipStream_t)stream;
    const CritWs w = crit_layout(const_cast<void*>(workspace_dev), batch, m, n, with_margin != 0);
    const int mx = m > n ? m : n;
    if (grad_scores) {
        hipError_t e = hipMemsetAsync(grad_scores, 0, sizeof(float) * (size_t)batch * (m + 1) * (n + 1), st);
        if (e != hipSuccess) return (int)e;
        hipLaunchKernelGGL(nll_grad_kernel, dim3((mx + 255) / 256, batch), dim3(256), 0, st, gt_matches0, gt_matches1, batch, m, n,
                           grad_losses, w, grad_scores);
    }
    if (want_desc) {
        hipError_t e = hipMemsetAsync(grad_context_descriptors0, 0, sizeof(float) * (size_t)batch * D * m, st);
        if (e == hipSuccess) e = hipMemsetAsync(grad_context_descriptors1, 0, sizeof(float) * (size_t)batch * D * n, st);
        if (e != hipSuccess) return (int)e;
        hipLaunchKernelGGL(metric_scatter_kernel, dim3((mx + 3) / 4, batch), dim3(256), 0, st, context_descriptors0, context_descriptors1,
                           gt_matches0, gt_matches1, batch, m, n, D, margin, grad_losses, w, grad_context_descriptors0,
                           grad_context_descriptors1);
        hipLaunchKernelGGL(normalize_grad_kernel, dim3((mx + 255) / 256, batch, 2), dim3(256), 0, st, context_descriptors0,
                           context_descriptors1, m, n, D, w, grad_context_descriptors0, grad_context_descriptors1);
    }
    return og_launch_status();
}
