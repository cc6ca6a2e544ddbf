// Uncalibrated geometric verification: what the reference's inference.py gets from cv2.findFundamentalMat (inference.py:214-235), for
// a whole SuperGlue.match batch, without calibration and without leaving the GPU.  The RANSAC itself (workspace, the four kernels, the
// launches) is og_ransac_hartley.h's, instantiated over the model struct Fundamental below, which holds what is particular to F.
//
//  * og_fundamental_7pt -- the seven-point minimal solver, fp64, one thread per problem:
//      ransac_solve_kernel<Fundamental>
//                         fundamental_7pt: the 2-d null space {F1, F2} of the 7 x 9 epipolar constraints (Gauss-Jordan with row
//                         pivoting, then Gram-Schmidt), the cubic det(a F1 + (1 - a) F2) = 0: one real root by bisection inside the
//                         Cauchy bound, the other two from the deflated quadratic, Newton on the cubic for each; a vanishing leading
//                         coefficient is the root at infinity, F = F1 - F2.  Roots in ascending order, the one at infinity last; a
//                         model is kept when the seven constraints and det F hold to 1e-9 at unit Frobenius norm.
//
//  * og_fundamental_matrix -- RANSAC over that solver, then least-squares refits, the skeleton's four launches with:
//      sample             7 matches, up to 3 models, the model index is hypothesis * 3 + solution
//      error              squared Sampson error in pixels^2 <= threshold^2 in fp32 on the normalised coordinates (the two scales
//                         enter the denominator)
//      refit              one epipolar constraint row per inlier; the eigenvector is made rank 2 through jacobi3 on F^T F
//      pixels             F = T1^T Fn T0
//
//  * og_fundamental_matrix_sc -- the same with sigma-consensus scoring, the SC = 1 instances of the score and finish kernels.
#include "og_common.h"
#include "og_ransac_hartley.h"

namespace {

constexpr int kFSlots = 27;         // doubles per problem in the F buffer: 3 models

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

// ------------------------------------------------------------------------------------------------ the model
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

struct Fundamental {
    static constexpr int kSample = 7, kSol = 3, kSlots = kFSlots;
    static __host__ __device__ __forceinline__ int solve(const double* x0, const double* x1, double* Fout) { return fundamental_7pt(x0, x1, Fout); }
    struct Pair { float bound, s0sq, s1sq; };
    static __device__ __forceinline__ Pair pair(float t2, double s0, double s1) { return {t2, (float)(s0 * s0), (float)(s1 * s1)}; }
    static __device__ __forceinline__ float error(const float (&e)[9], float4 q, const Pair& p) { return sampson_px(e, q, p.s0sq, p.s1sq); }
    // the epipolar constraint of the match, one row
    struct Rows { double r[9]; };
    static __device__ __forceinline__ Rows rows(double4 q) { return {{q.z * q.x, q.z * q.y, q.z, q.w * q.x, q.w * q.y, q.w, q.x, q.y, 1.0}}; }
    template <int SC>
    static __device__ __forceinline__ double term(const Rows& w, float wt, int i, int j) {
        const double (&r)[9] = w.r;
        const double ri = SC ? (double)wt * r[i] : r[i];      // the weighted row: one multiply per entry
        return ri * r[j];
    }
    static __device__ __forceinline__ bool polish(double (&F)[9]) { return rank2_unit(F); }
    // F = T1^T (Fn T0) with T = [[s 0 -s cx] [0 s -s cy] [0 0 1]]
    static __device__ __forceinline__ void to_pixels(const double (&G)[9], double s1, double cx1, double cy1, double (&Fp)[9]) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            Fp[c] = s1 * G[c];
            Fp[3 + c] = s1 * G[3 + c];
            Fp[6 + c] = G[6 + c] - s1 * (cx1 * G[c] + cy1 * G[3 + c]);
        }
    }
};

}  // namespace

// ------------------------------------------------------------------------------------------------ C ABI
extern "C" int og_fundamental_7pt(int32_t count, const double* x0, const double* x1, double* F, int32_t* num_solutions, void* stream) {
    og_clear_status();
    return minimal_solve<Fundamental>(count, x0, x1, F, num_solutions, stream);
}

extern "C" size_t og_fundamental_matrix_workspace_bytes(int32_t batch, int32_t m, int32_t hypotheses) {
    if (!ransac_sizes_ok<Fundamental>(batch, m, hypotheses)) return 0;
    return ransac_bytes<Fundamental>(batch, m, hypotheses);
}

extern "C" int og_fundamental_matrix(int32_t batch, int32_t m, int32_t n, const float* keypoints0, const float* keypoints1,
                                     const int64_t* matches0, const int32_t* num_keypoints0, float threshold, int32_t hypotheses,
                                     int32_t refine, uint64_t seed, int64_t pair_offset, double* F, uint8_t* inliers,
                                     int32_t* num_inliers, int32_t* best_model, void* workspace_dev, void* stream) {
    og_clear_status();
    return ransac_run<Fundamental, 0>(batch, m, n, keypoints0, keypoints1, matches0, num_keypoints0, threshold, hypotheses, refine, seed,
                                      pair_offset, F, inliers, num_inliers, best_model, workspace_dev, stream);
}

extern "C" int og_fundamental_matrix_sc(int32_t batch, int32_t m, int32_t n, const float* keypoints0, const float* keypoints1,
                                        const int64_t* matches0, const int32_t* num_keypoints0, float threshold, int32_t hypotheses,
                                        int32_t refine, uint64_t seed, int64_t pair_offset, double* F, uint8_t* inliers,
                                        int32_t* num_inliers, int32_t* best_model, float* quality, void* workspace_dev, void* stream) {
    og_clear_status();
    if (!quality) return OG_E_INVALID;
    if (m > kSigmaMaxMatches) return OG_E_SHAPE;
    return ransac_run<Fundamental, 1>(batch, m, n, keypoints0, keypoints1, matches0, num_keypoints0, threshold, hypotheses, refine, seed,
                                      pair_offset, F, inliers, num_inliers, best_model, workspace_dev, stream, quality);
}
