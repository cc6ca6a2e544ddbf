// Uncalibrated geometric verification: what the reference's inference.py gets from cv2.findFundamentalMat (inference.py:214-235), for
// a whole SuperGlue.match batch, without calibration and without leaving the GPU.
//
//  * og_fundamental_7pt -- the seven-point minimal solver, fp64, one thread per problem:
//      fm_solve_kernel    the 2-d null space {F1, F2} of the 7 x 9 epipolar constraints (Gauss-Jordan with row pivoting, then
//                         Gram-Schmidt), the cubic det(a F1 + (1 - a) F2) = 0: one real root by bisection inside the Cauchy bound,
//                         the other two from the deflated quadratic, Newton on the cubic for each; a vanishing leading coefficient
//                         is the root at infinity, F = F1 - F2.  Roots in ascending order, the one at infinity last; a model is
//                         kept when the seven constraints and det F hold to 1e-9 at unit Frobenius norm.
//
//  * og_fundamental_matrix -- RANSAC over that solver, then least-squares refits:
//      fm_prep_kernel     one workgroup per pair: the valid matches compacted in index order, Hartley normalisation of both images
//                         (centroid, mean distance sqrt 2) in fp64, summed over the COMPACTED order lanes-then-waves, so that a pair
//                         gives the same bits whatever holes or padding surround its matches
//      fm_solve_kernel    one thread per (pair, hypothesis): 7 distinct matches drawn by the counter-based hash of metrics.hip
//      fm_score_kernel    one model (hypothesis, solution) per lane, the pair's points staged through LDS, squared Sampson error in
//                         pixels^2 <= threshold^2 in fp32 on the normalised coordinates (the two scales enter the denominator); the
//                         winner per pair is a packed 64-bit atomicMax of (inliers + 1, ~model index)
//      fm_finish_kernel   one workgroup per pair: `refine` rounds of {the 45 distinct entries of the 9 x 9 normal matrix of the
//                         inliers' constraints in fp64 (lanes, then waves), its smallest eigenvector by cyclic Jacobi with one matrix
//                         row per lane, rank 2 through jacobi3 on F^T F, inliers recounted, kept if not fewer}, then the mask by the
//                         same fp32 test, F back in pixels, unit norm, largest entry positive
//    Four launches whatever the batch; no host synchronisation, no float atomics: every output is identical from run to run.
//
//  * og_fundamental_matrix_sc -- the same four launches with sigma-consensus scoring: the score and finish kernels are templates on
//    the scoring mode, this unit instantiates the hard count (SC = 0), and sigma_consensus.hip includes this file with OG_SIGMA_UNIT
//    for the SC = 1 instances and their entry.
#include "og_common.h"
#include "og_ransac.h"

namespace {

constexpr int kFSol = 3;            // models per hypothesis
constexpr int kFSlots = 27;         // doubles per problem in the F buffer
constexpr int kFChunk = 1024;       // points per LDS stage of the scorer

// ------------------------------------------------------------------------------------------------ seven-point solver
__host__ __device__ inline double det9(const double (&F)[9]) {
    return F[0] * (F[4] * F[8] - F[5] * F[7]) - F[1] * (F[3] * F[8] - F[5] * F[6]) + F[2] * (F[3] * F[7] - F[4] * F[6]);
}

// Up to three Newton steps on the cubic c (ascending), each kept only if it lowers |c(a)|
__host__ __device__ inline double cubic_polish(const double (&c)[4], double a) {
    double f = fabs(peval<4>(c, a));
#pragma unroll 1
    for (int it = 0; it < 3; ++it) {
        const double d = (3.0 * c[3] * a + 2.0 * c[2]) * a + c[1];
        const double an = a - peval<4>(c, a) / d;
        const double fn = fabs(peval<4>(c, an));
        if (!(fn < f)) break;
        a = an; f = fn;
    }
    return a;
}

// x0, x1: 7 points each ([7][2], coordinates of order 1).  Fout: up to three unit-norm F (row-major, x1^T F x0 = 0); the
// slots past the count are zeroed.  Returns the count.
__host__ __device__ inline int fundamental_7pt(const double* x0, const double* x1, double* Fout) {
#pragma unroll 1
    for (int c = 0; c < kFSlots; ++c) Fout[c] = 0.0;
    double Q[7][9];
#pragma unroll
    for (int r = 0; r < 7; ++r) {
        const double u0 = x0[2 * r], v0 = x0[2 * r + 1], u1 = x1[2 * r], v1 = x1[2 * r + 1];
        Q[r][0] = u1 * u0; Q[r][1] = u1 * v0; Q[r][2] = u1;
        Q[r][3] = v1 * u0; Q[r][4] = v1 * v0; Q[r][5] = v1;
        Q[r][6] = u0;      Q[r][7] = v0;      Q[r][8] = 1.0;
    }
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 7; ++k) {
#pragma unroll
        for (int r = k + 1; r < 7; ++r) {
            const bool sw = fabs(Q[r][k]) > fabs(Q[k][k]);
#pragma unroll
            for (int c = 0; c < 9; ++c) {
                const double a = Q[k][c], b = Q[r][c];
                Q[k][c] = sw ? b : a;
                Q[r][c] = sw ? a : b;
            }
        }
        const double piv = Q[k][k];
        ok = ok && fabs(piv) > 1e-300;
        const double inv = 1.0 / piv;
#pragma unroll
        for (int c = 0; c < 9; ++c) Q[k][c] *= inv;
#pragma unroll
        for (int r = 0; r < 7; ++r) {
            if (r == k) continue;
            const double f = Q[r][k];
#pragma unroll
            for (int c = 0; c < 9; ++c) Q[r][c] -= f * Q[k][c];
        }
    }
    if (!ok) return 0;
    // null space: free columns 7, 8; then modified Gram-Schmidt for conditioning
    double Nb[2][9];
#pragma unroll
    for (int f = 0; f < 2; ++f) {
#pragma unroll
        for (int p = 0; p < 7; ++p) Nb[f][p] = -Q[p][7 + f];
#pragma unroll
        for (int g = 0; g < 2; ++g) Nb[f][7 + g] = f == g ? 1.0 : 0.0;
    }
#pragma unroll
    for (int f = 0; f < 2; ++f) {
#pragma unroll
        for (int g = 0; g < f; ++g) {
            double d = 0.0;
#pragma unroll
            for (int c = 0; c < 9; ++c) d += Nb[f][c] * Nb[g][c];
#pragma unroll
            for (int c = 0; c < 9; ++c) Nb[f][c] -= d * Nb[g][c];
        }
        double n2 = 0.0;
#pragma unroll
        for (int c = 0; c < 9; ++c) n2 += Nb[f][c] * Nb[f][c];
        const double inv = 1.0 / sqrt(n2);
#pragma unroll
        for (int c = 0; c < 9; ++c) Nb[f][c] *= inv;
    }
    // F(a) = F2 + a D, D = F1 - F2: det F(a) = c0 + c1 a + c2 a^2 + c3 a^3
    double D[9];
#pragma unroll
    for (int c = 0; c < 9; ++c) D[c] = Nb[0][c] - Nb[1][c];
    typedef double P1[2];
    P1 e[9];
#pragma unroll
    for (int c = 0; c < 9; ++c) { e[c][0] = Nb[1][c]; e[c][1] = D[c]; }
    double c[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int t = 0; t < 3; ++t) {
        // cofactor expansion along the first row: e[t] * (e[3 + u] e[6 + v] - e[3 + v] e[6 + u]), (u, v) = the other two columns
        const int u = t == 0 ? 1 : 0, v = t == 2 ? 1 : 2;
        double m0[3], m1[3], term[4];
        pmul(e[3 + u], e[6 + v], m0);
        pmul(e[3 + v], e[6 + u], m1);
#pragma unroll
        for (int i = 0; i < 3; ++i) m0[i] -= m1[i];
        pmul(e[t], m0, term);
#pragma unroll
        for (int i = 0; i < 4; ++i) c[i] += t == 1 ? -term[i] : term[i];
    }
    const double cmax = fmax(fmax(fabs(c[0]), fabs(c[1])), fmax(fabs(c[2]), fabs(c[3])));
    if (!(cmax > 0.0) || !finite(cmax)) return 0;
    const double tiny = 1e-12 * cmax;
    double r0 = __builtin_huge_val(), r1 = r0, r2 = r0;          // finite roots; unused slots stay at +inf and sort last
    int nr = 0;
    bool at_inf = false;
    // the roots of t^2 + e1 t + e0, if real
    auto quadratic = [](double e1, double e0, double& ra, double& rb) {
        const double disc = e1 * e1 - 4.0 * e0;
        if (!(disc >= 0.0)) return 0;
        const double qq = -0.5 * (e1 + (e1 >= 0.0 ? 1.0 : -1.0) * sqrt(disc));
        ra = qq; rb = qq != 0.0 ? e0 / qq : 0.0;
        return 2;
    };
    if (fabs(c[3]) > tiny) {
        const double a2 = c[2] / c[3], a1 = c[1] / c[3], a0 = c[0] / c[3];
        const double bound = 1.0 + fmax(fabs(a2), fmax(fabs(a1), fabs(a0)));      // Cauchy: every root lies in (-bound, bound)
        const double mono[4] = {a0, a1, a2, 1.0};
        double lo = -bound, hi = bound;
#pragma unroll 1
        for (int it = 0; it < 200; ++it) {
            const double mid = 0.5 * (lo + hi);
            if (!(mid > lo && mid < hi)) break;
            if (peval<4>(mono, mid) > 0.0) hi = mid; else lo = mid;
        }
        r0 = cubic_polish(mono, 0.5 * (lo + hi));
        const double e1 = a2 + r0;
        nr = 1 + quadratic(e1, a1 + r0 * e1, r1, r2);
    } else {
        at_inf = true;
        if (fabs(c[2]) > tiny) nr = quadratic(c[1] / c[2], c[0] / c[2], r0, r1);
        else if (fabs(c[1]) > tiny) { r0 = -c[0] / c[1]; nr = 1; }
    }
    // ascending order: three compare-exchanges
    { const double a = fmin(r0, r1), b = fmax(r0, r1); r0 = a; r1 = b; }
    { const double a = fmin(r1, r2), b = fmax(r1, r2); r1 = a; r2 = b; }
    { const double a = fmin(r0, r1), b = fmax(r0, r1); r0 = a; r1 = b; }
    int nsol = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const bool inf_slot = j == 3;
        if (inf_slot ? !at_inf : j >= nr) continue;
        double F[9], n2 = 0.0;
        if (inf_slot) {
#pragma unroll
            for (int k = 0; k < 9; ++k) F[k] = D[k];
        } else {
            const double a = cubic_polish(c, j == 0 ? r0 : j == 1 ? r1 : r2);
#pragma unroll
            for (int k = 0; k < 9; ++k) F[k] = Nb[1][k] + a * D[k];
        }
#pragma unroll
        for (int k = 0; k < 9; ++k) n2 += F[k] * F[k];
        const double inv = 1.0 / sqrt(n2);
        if (!finite(inv)) continue;
#pragma unroll
        for (int k = 0; k < 9; ++k) F[k] *= inv;
        double worst = fabs(det9(F));
#pragma unroll
        for (int r = 0; r < 7; ++r) {
            const double u0 = x0[2 * r], v0 = x0[2 * r + 1], u1 = x1[2 * r], v1 = x1[2 * r + 1];
            const double s = u1 * (F[0] * u0 + F[1] * v0 + F[2]) + v1 * (F[3] * u0 + F[4] * v0 + F[5]) + (F[6] * u0 + F[7] * v0 + F[8]);
            worst = fmax(worst, fabs(s));
        }
        if (!(worst <= 1e-9)) continue;
#pragma unroll
        for (int k = 0; k < 9; ++k) Fout[nsol * 9 + k] = F[k];
        ++nsol;
    }
    return nsol;
}

// ------------------------------------------------------------------------------------------------ RANSAC
struct FGeo {
    const float* k0; const float* k1; const int64_t* matches0; const int32_t* nk0;
    int B, m, n;
};

struct FundWs {
    double4* pts;          // [B][m] the valid matches in index order, normalised (u0, v0, u1, v1)
    int* idx;              // [B][m] their keypoint0 index
    int* count;            // [B]
    double* norm;          // [B][6] centroid and scale of image 0, of image 1
    unsigned long long* best;   // [B] packed (inliers + 1, ~model)
    double* F;             // [B * H][27]
    int* nsol;             // [B * H]
};

static size_t fund_bytes(int B, int m, int H) {
    const int64_t bm = (int64_t)B * m, bh = (int64_t)B * H;
    return og_round_up(32 * bm, 256) + og_round_up(4 * bm, 256) + og_round_up(4 * (int64_t)B, 256) + og_round_up(48 * (int64_t)B, 256) +
           og_round_up(8 * (int64_t)B, 256) + og_round_up(8 * kFSlots * bh, 256) + og_round_up(4 * bh, 256);
}

static FundWs fund_layout(void* ws, int B, int m, int H) {
    FundWs w{};
    char* p = (char*)ws;
    const int64_t bm = (int64_t)B * m, bh = (int64_t)B * H;
    auto take = [&](int64_t bytes) { char* r = p; p += og_round_up(bytes, 256); return r; };
    w.pts = (double4*)take(32 * bm);
    w.idx = (int*)take(4 * bm);
    w.count = (int*)take(4 * (int64_t)B);
    w.norm = (double*)take(48 * (int64_t)B);
    w.best = (unsigned long long*)take(8 * (int64_t)B);
    w.F = (double*)take(8 * kFSlots * bh);
    w.nsol = (int*)take(4 * bh);
    return w;
}

__global__ void __launch_bounds__(256) fm_prep_kernel(FGeo g, FundWs w) { hartley_prep_pair(g, w); }

struct FSolveSrc {
    const double* x0; const double* x1;      // direct problems (og_fundamental_7pt): [count][7][2]
    const double4* pts; const int* cnt;      // RANSAC draws (og_fundamental_matrix): problem = b * H + h
    int m, H;
    uint64_t seed;
    int64_t pair_offset;
};

__global__ void __launch_bounds__(64) fm_solve_kernel(FSolveSrc src, int count, double* F, int* nsol) {
    const int p = blockIdx.x * 64 + threadIdx.x;
    if (p >= count) return;
    double x0[14], x1[14];
    if (src.x0) {
#pragma unroll
        for (int i = 0; i < 14; ++i) { x0[i] = src.x0[(int64_t)p * 14 + i]; x1[i] = src.x1[(int64_t)p * 14 + i]; }
    } else {
        const int b = p / src.H, h = p - b * src.H;
        const int n = src.cnt[b];
        if (n < 7) { nsol[p] = 0; return; }
        int pick[7];
        draw_distinct<7>(src.seed, (uint64_t)(src.pair_offset + b), h, n, pick);
#pragma unroll
        for (int j = 0; j < 7; ++j) {
            const double4 q = src.pts[(int64_t)b * src.m + pick[j]];
            x0[2 * j] = q.x; x0[2 * j + 1] = q.y; x1[2 * j] = q.z; x1[2 * j + 1] = q.w;
        }
    }
    nsol[p] = fundamental_7pt(x0, x1, F + (int64_t)p * kFSlots);
}

// Squared Sampson error in pixels^2 <= t2 on normalised coordinates q = (u0, v0, u1, v1), x_pixel = x / s + c: the numerator
// x1^T F x0 is the same in both frames, the gradient of image 0 carries that image's scale s0 and likewise s1 (s0sq, s1sq: the squares).
// fp32, explicit FMAs: the score and finish kernels agree bitwise.  sampson_px is the error, which sigma-consensus scoring weighs.
__device__ __forceinline__ float sampson_px(const float (&e)[9], float4 q, float s0sq, float s1sq) {
    const float a0 = __fmaf_rn(e[0], q.x, __fmaf_rn(e[1], q.y, e[2]));
    const float a1 = __fmaf_rn(e[3], q.x, __fmaf_rn(e[4], q.y, e[5]));
    const float a2 = __fmaf_rn(e[6], q.x, __fmaf_rn(e[7], q.y, e[8]));
    const float b0 = __fmaf_rn(e[0], q.z, __fmaf_rn(e[3], q.w, e[6]));
    const float b1 = __fmaf_rn(e[1], q.z, __fmaf_rn(e[4], q.w, e[7]));
    const float num = __fmaf_rn(q.z, a0, __fmaf_rn(q.w, a1, a2));
    const float g1 = __fmaf_rn(a0, a0, __fmul_rn(a1, a1));        // |d/dx1|^2 / s1^2
    const float g0 = __fmaf_rn(b0, b0, __fmul_rn(b1, b1));        // |d/dx0|^2 / s0^2
    const float den = __fmaf_rn(s1sq, g1, __fmul_rn(s0sq, g0));
    return __fdiv_rn(__fmul_rn(num, num), den);
}
__device__ __forceinline__ bool sampson_inlier_px(const float (&e)[9], float4 q, float s0sq, float s1sq, float t2) {
    return sampson_px(e, q, s0sq, s1sq) <= t2;
}

// SC = 0: a model's score is its number of inliers.  SC = 1: sigma-consensus, the score is Q = sum of q in units of 2^-16 (og_ransac.h).
template <int SC>
__global__ void __launch_bounds__(256) fm_score_kernel(FundWs w, int m, int H, int groups, float t2) {
    __shared__ float4 pts[kFChunk];
    const float* sig = nullptr;
    if constexpr (SC) {
        __shared__ float tab[kSigmaCells + 1];
        sigma_table_fill(tab);                               // the barriers of the first chunk come before its first use
        sig = tab;
    }
    const int b = blockIdx.x / groups;                       // `groups` workgroups per pair, pair-major along x
    const int model = (blockIdx.x - b * groups) * 256 + threadIdx.x;        // h * 3 + s
    const int h = model / kFSol, s = model - h * kFSol;
    const int64_t prob = (int64_t)b * H + h;
    const bool live = h < H && s < w.nsol[h < H ? prob : 0];
    float e[9];
#pragma unroll
    for (int c = 0; c < 9; ++c) e[c] = live ? (float)w.F[prob * kFSlots + s * 9 + c] : 0.0f;
    const int n = w.count[b];
    const float s0sq = (float)(w.norm[(int64_t)b * 6 + 2] * w.norm[(int64_t)b * 6 + 2]), s1sq = (float)(w.norm[(int64_t)b * 6 + 5] * w.norm[(int64_t)b * 6 + 5]);
    const float inv_t2 = sigma_inv_bound(t2);                // SC = 1 only
    int inl = 0;
    uint32_t Q = 0u;
    for (int k0 = 0; k0 < n; k0 += kFChunk) {
        const int len = min(kFChunk, n - k0);
        __syncthreads();
        for (int k = threadIdx.x; k < len; k += 256) pts[k] = to_f4(w.pts[(int64_t)b * m + k0 + k]);
        __syncthreads();
        if constexpr (SC) {
            if (live)
#pragma unroll 4
                for (int k = 0; k < len; ++k) {
                    uint32_t q;
                    float wt;
                    sigma_match(sig, sampson_px(e, pts[k], s0sq, s1sq), t2, inv_t2, q, wt);
                    Q += q;
                }
        } else {
            if (live)
                for (int k = 0; k < len; ++k) inl += sampson_inlier_px(e, pts[k], s0sq, s1sq, t2);
        }
    }
    const unsigned long long score = SC ? (unsigned long long)Q : (unsigned long long)inl;
    const unsigned long long key = live ? ((score + 1) << 32) | (unsigned)(0xFFFFFFFFu - (unsigned)model) : 0ull;
    publish_best(key, &w.best[b]);
}

// F (row-major, any scale) -> the nearest rank-2 matrix at unit Frobenius norm: the right singular vector of the smallest singular
// value (jacobi3 on F^T F) is projected out.  false if the result is not finite.
__device__ inline bool rank2_unit(double (&F)[9]) {
    double A[3][3], V[3][3];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) A[r][c] = F[r] * F[c] + F[3 + r] * F[3 + c] + F[6 + r] * F[6 + c];
    jacobi3(A, V);
    const int lo = (A[0][0] <= A[1][1] && A[0][0] <= A[2][2]) ? 0 : (A[1][1] <= A[2][2] ? 1 : 2);
    double vm[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) vm[r] = lo == 0 ? V[r][0] : lo == 1 ? V[r][1] : V[r][2];
    double n2 = 0.0;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const double fv = F[r * 3] * vm[0] + F[r * 3 + 1] * vm[1] + F[r * 3 + 2] * vm[2];
#pragma unroll
        for (int c = 0; c < 3; ++c) { F[r * 3 + c] -= fv * vm[c]; n2 += F[r * 3 + c] * F[r * 3 + c]; }
    }
    const double inv = 1.0 / sqrt(n2);
#pragma unroll
    for (int c = 0; c < 9; ++c) F[c] *= inv;
    return finite(inv);
}

// SC as in fm_score_kernel.  SC = 1: the refit's rows are weighted by w, a refit is kept if its Q is no smaller, and the last argument
// is `float* quality`, Q / 65536 of the final model.
template <int SC, class... Quality>
__global__ void __launch_bounds__(256) fm_finish_kernel(FGeo g, FundWs w, int H, int refine, float t2, double* F_out, uint8_t* inliers,
                                                        int* num_inliers, int* best_model, Quality... quality) {
    const float* sig = nullptr;
    if constexpr (SC) {
        __shared__ float tab[kSigmaCells + 1];
        sigma_table_fill(tab);
        __syncthreads();
        sig = tab;
    }
    __shared__ double racc[4][45];
    __shared__ double fnew[10];          // the refit and 1.0 if it is sound
    __shared__ int red[4];
    const int b = blockIdx.x, lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int n = w.count[b];
    const unsigned long long key = w.best[b];
    const bool have = key != 0ull && n >= 7;
    const int model = (int)(0xFFFFFFFFu - (unsigned)(key & 0xFFFFFFFFull));
    const int h = model / kFSol, s = model - h * kFSol;
    const double4* P = w.pts + (int64_t)b * g.m;
    for (int i = threadIdx.x; i < g.m; i += 256) inliers[(int64_t)b * g.m + i] = 0;
    if (!have) {
        if (threadIdx.x == 0) {
#pragma unroll
            for (int c = 0; c < 9; ++c) F_out[(int64_t)b * 9 + c] = 0.0;
            num_inliers[b] = 0;
            best_model[b] = -1;
            store_quality(b, 0.0f, quality...);
        }
        return;
    }
    const double s0 = w.norm[(int64_t)b * 6 + 2], s1 = w.norm[(int64_t)b * 6 + 5];
    const float s0sq = (float)(s0 * s0), s1sq = (float)(s1 * s1);
    double Fc[9];
    float e[9];
#pragma unroll
    for (int c = 0; c < 9; ++c) { Fc[c] = w.F[((int64_t)b * H + h) * kFSlots + s * 9 + c]; e[c] = (float)Fc[c]; }
    const float inv_t2 = sigma_inv_bound(t2);                // SC = 1 only
    auto count_inliers = [&](const float (&f)[9]) {
        int c = 0;
        for (int k = threadIdx.x; k < n; k += 256) c += sampson_inlier_px(f, to_f4(P[k]), s0sq, s1sq, t2);
        return block_sum(c, red);
    };
    // sigma-consensus: the inliers of a model to cnt and its Q returned, one pass
    auto measure = [&](const float (&f)[9], int& cnt) {
        int c = 0;
        uint32_t Q = 0u;
        for (int k = threadIdx.x; k < n; k += 256) {
            uint32_t q;
            float wt;
            c += sigma_match(sig, sampson_px(f, to_f4(P[k]), s0sq, s1sq), t2, inv_t2, q, wt);
            Q += q;
        }
        cnt = block_sum(c, red);
        return block_sum(Q, (uint32_t*)red);
    };
    int cur;
    uint32_t curq = 0u;
    if constexpr (SC) curq = measure(e, cur); else cur = count_inliers(e);
    for (int round = 0; round < refine; ++round) {
        if (cur < 8) break;
        double acc[45];
#pragma unroll
        for (int c = 0; c < 45; ++c) acc[c] = 0.0;
        for (int k = threadIdx.x; k < n; k += 256) {
            const double4 q = P[k];
            uint32_t qk;
            float wt;
            if constexpr (SC) {
                if (!sigma_match(sig, sampson_px(e, to_f4(q), s0sq, s1sq), t2, inv_t2, qk, wt)) continue;
            } else {
                if (!sampson_inlier_px(e, to_f4(q), s0sq, s1sq, t2)) continue;
            }
            const double r[9] = {q.z * q.x, q.z * q.y, q.z, q.w * q.x, q.w * q.y, q.w, q.x, q.y, 1.0};
#pragma unroll
            for (int i = 0; i < 9; ++i) {
                const double ri = SC ? (double)wt * r[i] : r[i];      // the weighted row: one multiply per entry
#pragma unroll
                for (int j = i; j < 9; ++j) acc[tri(i, j)] += ri * r[j];
            }
        }
#pragma unroll
        for (int c = 0; c < 45; ++c) {
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) acc[c] += __shfl_xor(acc[c], o, 64);
        }
        __syncthreads();
        if (lane == 0)
#pragma unroll
            for (int c = 0; c < 45; ++c) racc[wid][c] = acc[c];
        __syncthreads();
        if (wid == 0) {
            double a[9], v[9];
#pragma unroll
            for (int j = 0; j < 9; ++j) {
                const int t = tri(lane < 9 ? lane : 0, j);
                const double sum = ((racc[0][t] + racc[1][t]) + racc[2][t]) + racc[3][t];
                a[j] = lane < 9 ? sum : 0.0;
            }
            jacobi9_wave(a, v, lane);
            // the smallest eigenvalue: lowest index on ties
            double ev = 0.0;
#pragma unroll
            for (int j = 0; j < 9; ++j) ev = lane == j ? a[j] : ev;
            int jm = 0;
            double em = __shfl(ev, 0, 64);
#pragma unroll
            for (int j = 1; j < 9; ++j) {
                const double ej = __shfl(ev, j, 64);
                if (ej < em) { em = ej; jm = j; }
            }
            double col = 0.0;
#pragma unroll
            for (int j = 0; j < 9; ++j) col = jm == j ? v[j] : col;
            double Fr[9];
#pragma unroll
            for (int k = 0; k < 9; ++k) Fr[k] = __shfl(col, k, 64);
            const bool sound = rank2_unit(Fr);
            if (lane == 0) {
#pragma unroll
                for (int k = 0; k < 9; ++k) fnew[k] = Fr[k];
                fnew[9] = sound ? 1.0 : 0.0;
            }
        }
        __syncthreads();
        double Fn[9];
        float en[9];
#pragma unroll
        for (int c = 0; c < 9; ++c) { Fn[c] = fnew[c]; en[c] = (float)Fn[c]; }
        const bool sound = fnew[9] == 1.0;
        int cnt;                                        // the count's barriers also keep fnew until every lane has read it
        uint32_t qn = 0u;
        if constexpr (SC) qn = measure(en, cnt); else cnt = count_inliers(en);
        if (sound && (SC ? qn >= curq : cnt >= cur)) {
            cur = cnt;
            curq = qn;
#pragma unroll
            for (int c = 0; c < 9; ++c) { Fc[c] = Fn[c]; e[c] = en[c]; }
        }
    }
    __syncthreads();                                    // the zeros above are in memory before the flags
    for (int k = threadIdx.x; k < n; k += 256)
        if (sampson_inlier_px(e, to_f4(P[k]), s0sq, s1sq, t2)) inliers[(int64_t)b * g.m + w.idx[(int64_t)b * g.m + k]] = 1;
    if (threadIdx.x != 0) return;
    // pixels: F = T1^T Fn T0 with T = [[s 0 -s cx] [0 s -s cy] [0 0 1]]
    const double cx0 = w.norm[(int64_t)b * 6 + 0], cy0 = w.norm[(int64_t)b * 6 + 1], cx1 = w.norm[(int64_t)b * 6 + 3], cy1 = w.norm[(int64_t)b * 6 + 4];
    double G[9], Fp[9];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        G[r * 3] = s0 * Fc[r * 3];
        G[r * 3 + 1] = s0 * Fc[r * 3 + 1];
        G[r * 3 + 2] = Fc[r * 3 + 2] - s0 * (cx0 * Fc[r * 3] + cy0 * Fc[r * 3 + 1]);
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        Fp[c] = s1 * G[c];
        Fp[3 + c] = s1 * G[3 + c];
        Fp[6 + c] = G[6 + c] - s1 * (cx1 * G[c] + cy1 * G[3 + c]);
    }
    double n2 = 0.0, big = 0.0;
#pragma unroll
    for (int c = 0; c < 9; ++c) { n2 += Fp[c] * Fp[c]; big = fabs(Fp[c]) > fabs(big) ? Fp[c] : big; }
    double inv = 1.0 / sqrt(n2);
    inv = finite(inv) ? (big < 0.0 ? -inv : inv) : 0.0;
#pragma unroll
    for (int c = 0; c < 9; ++c) F_out[(int64_t)b * 9 + c] = Fp[c] * inv;
    num_inliers[b] = cur;
    best_model[b] = model;
    store_quality(b, (float)((double)curq / 65536.0), quality...);
}

}  // namespace

// ------------------------------------------------------------------------------------------------ C ABI
static bool fund_sizes_ok(int32_t batch, int32_t m, int32_t hypotheses) {
    return batch > 0 && m >= 0 && hypotheses > 0 && (int64_t)kFSol * batch * hypotheses <= (1 << 30);
}

// The four launches of og_fundamental_matrix (SC = 0) and og_fundamental_matrix_sc (SC = 1, quality = one float*).
template <int SC, class... Quality>
static int fund_run(int32_t batch, int32_t m, int32_t n, const float* keypoints0, const float* keypoints1, const int64_t* matches0,
                    const int32_t* num_keypoints0, float threshold, int32_t hypotheses, int32_t refine, uint64_t seed, int64_t pair_offset,
                    double* F, uint8_t* inliers, int32_t* num_inliers, int32_t* best_model, void* workspace_dev, void* stream,
                    Quality... quality) {
    if (!fund_sizes_ok(batch, m, hypotheses) || n < 0 || refine < 0 || !(threshold >= 0.0f) || !F || !num_inliers || !best_model ||
        !workspace_dev)
        return OG_E_INVALID;
    if (m > 0 && (!keypoints0 || !matches0 || !inliers || (n > 0 && !keypoints1))) return OG_E_INVALID;
    if ((uintptr_t)workspace_dev % 16) return OG_E_ALIGN;
    const FGeo g{keypoints0, keypoints1, matches0, num_keypoints0, batch, m, n};
    FundWs w = fund_layout(workspace_dev, batch, m, hypotheses);
    hipStream_t st = (hipStream_t)stream;
    const int count = batch * hypotheses;
    const float t2 = threshold * threshold;
    FSolveSrc src{};
    src.pts = w.pts; src.cnt = w.count; src.m = m; src.H = hypotheses; src.seed = seed; src.pair_offset = pair_offset;
    hipLaunchKernelGGL(fm_prep_kernel, dim3(batch), dim3(256), 0, st, g, w);
    hipLaunchKernelGGL(fm_solve_kernel, dim3((count + 63) / 64), dim3(64), 0, st, src, count, w.F, w.nsol);
    const int groups = (hypotheses * kFSol + 255) / 256;      // batch * groups <= 2^22 + batch by the size rule: one grid dimension
    hipLaunchKernelGGL(fm_score_kernel<SC>, dim3(batch * groups), dim3(256), 0, st, w, m, hypotheses, groups, t2);
    hipLaunchKernelGGL((fm_finish_kernel<SC, Quality...>), dim3(batch), dim3(256), 0, st, g, w, hypotheses, refine, t2, F, inliers,
                       num_inliers, best_model, quality...);
    return og_launch_status();
}

#ifdef OG_SIGMA_UNIT      // sigma_consensus.hip includes this file for the SC = 1 instances, so that this unit holds the four kernels it held
extern "C" int og_fundamental_matrix_sc(int32_t batch, int32_t m, int32_t n, const float* keypoints0, const float* keypoints1,
                                        const int64_t* matches0, const int32_t* num_keypoints0, float threshold, int32_t hypotheses,
                                        int32_t refine, uint64_t seed, int64_t pair_offset, double* F, uint8_t* inliers,
                                        int32_t* num_inliers, int32_t* best_model, float* quality, void* workspace_dev, void* stream) {
    og_clear_status();
    if (!quality) return OG_E_INVALID;
    if (m > kSigmaMaxMatches) return OG_E_SHAPE;
    return fund_run<1>(batch, m, n, keypoints0, keypoints1, matches0, num_keypoints0, threshold, hypotheses, refine, seed, pair_offset, F,
                       inliers, num_inliers, best_model, workspace_dev, stream, quality);
}
#else
extern "C" int og_fundamental_7pt(int32_t count, const double* x0, const double* x1, double* F, int32_t* num_solutions, void* stream) {
    og_clear_status();
    if (count <= 0 || count > (1 << 30) || !x0 || !x1 || !F || !num_solutions) return OG_E_INVALID;
    FSolveSrc src{};
    src.x0 = x0; src.x1 = x1;
    hipLaunchKernelGGL(fm_solve_kernel, dim3((count + 63) / 64), dim3(64), 0, (hipStream_t)stream, src, count, F, num_solutions);
    return og_launch_status();
}

extern "C" size_t og_fundamental_matrix_workspace_bytes(int32_t batch, int32_t m, int32_t hypotheses) {
    if (!fund_sizes_ok(batch, m, hypotheses)) return 0;
    return fund_bytes(batch, m, hypotheses);
}

extern "C" int og_fundamental_matrix(int32_t batch, int32_t m, int32_t n, const float* keypoints0, const float* keypoints1,
                                     const int64_t* matches0, const int32_t* num_keypoints0, float threshold, int32_t hypotheses,
                                     int32_t refine, uint64_t seed, int64_t pair_offset, double* F, uint8_t* inliers,
                                     int32_t* num_inliers, int32_t* best_model, void* workspace_dev, void* stream) {
    og_clear_status();
    return fund_run<0>(batch, m, n, keypoints0, keypoints1, matches0, num_keypoints0, threshold, hypotheses, refine, seed, pair_offset, F,
                       inliers, num_inliers, best_model, workspace_dev, stream);
}
#endif
