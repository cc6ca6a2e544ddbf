// Planar geometric verification and the validation metrics of the homography pre-training stage: what a user of cv2.findHomography
// gets for a planar scene, for a whole SuperGlue.match batch, without leaving the GPU, and the perspective counterparts of
// og_epipolar_precision / og_relative_pose's error (the reference validates nothing after pretrain_homography.py).  The RANSAC itself
// (workspace, the four kernels, the launches) is og_ransac_hartley.h's, instantiated over the model struct Homography below, which
// holds what is particular to H.
//
//  * og_homography_4pt -- the four-point minimal solver, fp64, one thread per problem:
//      ransac_solve_kernel<Homography>
//                         homography_4pt: the 8 x 9 DLT system of the four correspondences (Gauss-Jordan with row pivoting, the free
//                         column is the last), unit Frobenius norm, largest-magnitude entry positive.  A sample yields a model only if
//                         every one of its four point triples has a signed area above 1e-9 in both images with the same sign in both
//                         (cv2's orientation test; it removes collinear triples too), all nine entries are finite and the eight
//                         constraints hold to 1e-9.
//
//  * og_homography -- RANSAC over that solver, then least-squares refits, the skeleton's four launches with:
//      sample             4 matches, at most one model, the model index is the hypothesis
//      error              squared forward transfer error of x0 -> x1 in pixels^2 <= threshold^2 in fp32 on the normalised coordinates
//                         (image 1's scale enters the bound)
//      refit              the two DLT rows of every inlier; the eigenvector is taken to unit norm
//      pixels             H = T1^-1 Hn T0
//
//  * og_homography_sc -- the same with sigma-consensus scoring, the SC = 1 instances of the score and finish kernels.
//
//  * og_homography_precision -- hm_precision_kernel: per pair, |proj(H_true, k0[i]) - k1[matches0[i]]| in fp64 for every valid match
//  * og_homography_corner_error -- hm_corner_error_kernel: mean distance of the four image corners under the estimate and the truth
#include "og_common.h"
#include "og_ransac_hartley.h"

namespace {

constexpr int kHSlots = 9;          // doubles per problem in the H buffer

// ------------------------------------------------------------------------------------------------ four-point solver
// twice the signed area of the triangle (i, j, k) of x ([4][2])
__host__ __device__ inline double area2(const double* x, int i, int j, int k) {
    return (x[2 * j] - x[2 * i]) * (x[2 * k + 1] - x[2 * i + 1]) - (x[2 * j + 1] - x[2 * i + 1]) * (x[2 * k] - x[2 * i]);
}

// x0, x1: 4 points each ([4][2], coordinates of order 1).  Hout: the unit-norm H (row-major, x1 ~ H x0), zero without a model.
// Returns the count, 0 or 1.  No contraction in here: finite(v) is v - v == 0, and for a product v = a * b the compiler would fuse
// that into fma(a, b, -v), the product's rounding error, which is not zero for a finite v.
__host__ __device__ inline int homography_4pt(const double* x0, const double* x1, double* Hout) {
#pragma clang fp contract(off)
#pragma unroll 1
    for (int c = 0; c < kHSlots; ++c) Hout[c] = 0.0;
    bool ok = true;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        // the triple that leaves point t out
        const int i = t == 0 ? 1 : 0, j = t <= 1 ? 2 : 1, k = t <= 2 ? 3 : 2;
        const double a0 = area2(x0, i, j, k), a1 = area2(x1, i, j, k);
        ok = ok && fabs(a0) > 1e-9 && fabs(a1) > 1e-9 && (a0 > 0.0) == (a1 > 0.0);
    }
    double Q[8][9];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const double u0 = x0[2 * r], v0 = x0[2 * r + 1], u1 = x1[2 * r], v1 = x1[2 * r + 1];
        Q[2 * r][0] = u0;  Q[2 * r][1] = v0;  Q[2 * r][2] = 1.0;
        Q[2 * r][3] = 0.0; Q[2 * r][4] = 0.0; Q[2 * r][5] = 0.0;
        Q[2 * r][6] = -u1 * u0; Q[2 * r][7] = -u1 * v0; Q[2 * r][8] = -u1;
        Q[2 * r + 1][0] = 0.0; Q[2 * r + 1][1] = 0.0; Q[2 * r + 1][2] = 0.0;
        Q[2 * r + 1][3] = u0;  Q[2 * r + 1][4] = v0;  Q[2 * r + 1][5] = 1.0;
        Q[2 * r + 1][6] = -v1 * u0; Q[2 * r + 1][7] = -v1 * v0; Q[2 * r + 1][8] = -v1;
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) {
#pragma unroll
        for (int r = k + 1; r < 8; ++r) {
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
        for (int r = 0; r < 8; ++r) {
            if (r == k) continue;
            const double f = Q[r][k];
#pragma unroll
            for (int c = 0; c < 9; ++c) Q[r][c] -= f * Q[k][c];
        }
    }
    if (!ok) return 0;
    // null space: the free column is 8
    double Hm[9], n2 = 1.0, big = 1.0;
    Hm[8] = 1.0;
#pragma unroll
    for (int p = 0; p < 8; ++p) {
        Hm[p] = -Q[p][8];
        n2 += Hm[p] * Hm[p];
        big = fabs(Hm[p]) > fabs(big) ? Hm[p] : big;
    }
    double inv = 1.0 / sqrt(n2);
    inv = big < 0.0 ? -inv : inv;
    bool fin = finite(inv);
#pragma unroll
    for (int c = 0; c < 9; ++c) { Hm[c] *= inv; fin = fin && finite(Hm[c]); }
    if (!fin) return 0;
    double worst = 0.0;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const double u0 = x0[2 * r], v0 = x0[2 * r + 1], u1 = x1[2 * r], v1 = x1[2 * r + 1];
        const double px = Hm[0] * u0 + Hm[1] * v0 + Hm[2], py = Hm[3] * u0 + Hm[4] * v0 + Hm[5], pw = Hm[6] * u0 + Hm[7] * v0 + Hm[8];
        worst = fmax(worst, fmax(fabs(px - u1 * pw), fabs(py - v1 * pw)));
    }
    if (!(worst <= 1e-9)) return 0;
#pragma unroll
    for (int c = 0; c < 9; ++c) Hout[c] = Hm[c];
    return 1;
}

// ------------------------------------------------------------------------------------------------ the model
// Squared forward transfer error |proj(H, x0) - x1|^2 <= t2s on normalised coordinates q = (u0, v0, u1, v1), x_pixel = x / s + c: a
// distance in image 1 in pixels is the normalised one over s1, so t2s = threshold^2 s1^2.  A non-finite error (a point on the
// line H sends to infinity) compares false.  fp32, explicit FMAs: the score and finish kernels agree bitwise.  transfer_px is the
// error, which sigma-consensus scoring weighs.
__device__ __forceinline__ float transfer_px(const float (&e)[9], float4 q) {
    const float px = __fmaf_rn(e[0], q.x, __fmaf_rn(e[1], q.y, e[2]));
    const float py = __fmaf_rn(e[3], q.x, __fmaf_rn(e[4], q.y, e[5]));
    const float pw = __fmaf_rn(e[6], q.x, __fmaf_rn(e[7], q.y, e[8]));
    const float iw = __fdiv_rn(1.0f, pw);
    const float dx = __fmaf_rn(px, iw, -q.z), dy = __fmaf_rn(py, iw, -q.w);
    return __fmaf_rn(dx, dx, __fmul_rn(dy, dy));
}

// threshold^2 s1^2 in fp32, the one rounding both kernels use
__device__ __forceinline__ float transfer_bound(float t2, double s1) { return __fmul_rn(t2, (float)(s1 * s1)); }

struct Homography {
    static constexpr int kSample = 4, kSol = 1, kSlots = kHSlots;
    static __host__ __device__ __forceinline__ int solve(const double* x0, const double* x1, double* Hout) { return homography_4pt(x0, x1, Hout); }
    struct Pair { float bound; };
    static __device__ __forceinline__ Pair pair(float t2, double, double s1) { return {transfer_bound(t2, s1)}; }
    static __device__ __forceinline__ float error(const float (&e)[9], float4 q, const Pair&) { return transfer_px(e, q); }
    // the two DLT rows of the match: (x0^T, 0, -u1 x0^T) and (0, x0^T, -v1 x0^T)
    struct Rows { double ra[9], rb[9]; };
    static __device__ __forceinline__ Rows rows(double4 q) {
        return {{q.x, q.y, 1.0, 0.0, 0.0, 0.0, -q.z * q.x, -q.z * q.y, -q.z}, {0.0, 0.0, 0.0, q.x, q.y, 1.0, -q.w * q.x, -q.w * q.y, -q.w}};
    }
    template <int SC>
    static __device__ __forceinline__ double term(const Rows& w, float wt, int i, int j) {
        const double (&ra)[9] = w.ra, (&rb)[9] = w.rb;
        const double ai = SC ? (double)wt * ra[i] : ra[i], bi = SC ? (double)wt * rb[i] : rb[i];      // the weighted rows
        return ai * ra[j] + bi * rb[j];
    }
    static __device__ __forceinline__ bool polish(double (&Hr)[9]) {
        double n2 = 0.0;
#pragma unroll
        for (int k = 0; k < 9; ++k) n2 += Hr[k] * Hr[k];
        const double inv = 1.0 / sqrt(n2);
#pragma unroll
        for (int k = 0; k < 9; ++k) Hr[k] = Hr[k] * inv;
        return finite(inv);
    }
    // H = T1^-1 (Hn T0) with T = [[s 0 -s cx] [0 s -s cy] [0 0 1]], T^-1 = [[1/s 0 cx] [0 1/s cy] [0 0 1]]
    static __device__ __forceinline__ void to_pixels(const double (&G)[9], double s1, double cx1, double cy1, double (&Hp)[9]) {
        const double is1 = 1.0 / s1;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            Hp[c] = is1 * G[c] + cx1 * G[6 + c];
            Hp[3 + c] = is1 * G[3 + c] + cy1 * G[6 + c];
            Hp[6 + c] = G[6 + c];
        }
    }
};

// ------------------------------------------------------------------------------------------------ metrics
// (x, y) under the row-major 3 x 3 Hm, fp64; a point at infinity gives inf or NaN
__device__ inline void project(const double (&Hm)[9], double x, double y, double& u, double& v) {
    const double pw = Hm[6] * x + Hm[7] * y + Hm[8];
    u = (Hm[0] * x + Hm[1] * y + Hm[2]) / pw;
    v = (Hm[3] * x + Hm[4] * y + Hm[5]) / pw;
}

__global__ void __launch_bounds__(256) hm_precision_kernel(MatchGeo g, const float* H_true, float threshold, float* precision,
                                                           float* matching_score, int* num_correct) {
#pragma clang fp contract(off)
    __shared__ int red[4];
    const int b = blockIdx.x;
    double Ht[9];
#pragma unroll
    for (int c = 0; c < 9; ++c) Ht[c] = (double)H_true[(int64_t)b * 9 + c];
    int matched = 0, correct = 0;
    for (int i = threadIdx.x; i < g.m; i += blockDim.x) {
        int j;
        if (!valid_match(g, b, i, j)) continue;
        const float2 a = ((const float2*)g.k0)[(int64_t)b * g.m + i];
        const float2 c = ((const float2*)g.k1)[(int64_t)b * g.n + j];
        double u, v;
        project(Ht, (double)a.x, (double)a.y, u, v);
        const double dx = u - (double)c.x, dy = v - (double)c.y;
        ++matched;
        correct += sqrt(dx * dx + dy * dy) < (double)threshold;
    }
    matched = block_sum(matched, red);
    correct = block_sum(correct, red);
    if (threadIdx.x == 0) {
        const int det = g.nk0 ? min(g.nk0[b], g.m) : g.m;
        precision[b] = matched > 0 ? (float)correct / (float)matched : 0.0f;
        matching_score[b] = matched > 0 ? (float)correct / (float)det : 0.0f;
        num_correct[b] = correct;
    }
}

__global__ void __launch_bounds__(64) hm_corner_error_kernel(int B, const double* H_est, const float* H_true, int width, int height,
                                                             float* error) {
#pragma clang fp contract(off)
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= B) return;
    double He[9], Ht[9];
    bool any = false;
#pragma unroll
    for (int c = 0; c < 9; ++c) {
        He[c] = H_est[(int64_t)b * 9 + c];
        Ht[c] = (double)H_true[(int64_t)b * 9 + c];
        any = any || He[c] != 0.0;
    }
    double sum = 0.0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const double x = k < 2 ? 0.0 : (double)(width - 1), y = (k & 1) ? (double)(height - 1) : 0.0;
        double ue, ve, ut, vt;
        project(He, x, y, ue, ve);
        project(Ht, x, y, ut, vt);
        sum += sqrt((ue - ut) * (ue - ut) + (ve - vt) * (ve - vt));
    }
    const double mean = 0.25 * sum;
    error[b] = (any && finite(mean)) ? (float)mean : __builtin_huge_valf();
}

}  // namespace

// ------------------------------------------------------------------------------------------------ C ABI
extern "C" int og_homography_4pt(int32_t count, const double* x0, const double* x1, double* H, int32_t* num_solutions, void* stream) {
    og_clear_status();
    return minimal_solve<Homography>(count, x0, x1, H, num_solutions, stream);
}

extern "C" size_t og_homography_workspace_bytes(int32_t batch, int32_t m, int32_t hypotheses) {
    if (!ransac_sizes_ok<Homography>(batch, m, hypotheses)) return 0;
    return ransac_bytes<Homography>(batch, m, hypotheses);
}

extern "C" int og_homography(int32_t batch, int32_t m, int32_t n, const float* keypoints0, const float* keypoints1,
                             const int64_t* matches0, const int32_t* num_keypoints0, float threshold, int32_t hypotheses,
                             int32_t refine, uint64_t seed, int64_t pair_offset, double* H, uint8_t* inliers, int32_t* num_inliers,
                             int32_t* best_model, void* workspace_dev, void* stream) {
    og_clear_status();
    return ransac_run<Homography, 0>(batch, m, n, keypoints0, keypoints1, matches0, num_keypoints0, threshold, hypotheses, refine, seed,
                                     pair_offset, H, inliers, num_inliers, best_model, workspace_dev, stream);
}

extern "C" int og_homography_sc(int32_t batch, int32_t m, int32_t n, const float* keypoints0, const float* keypoints1,
                                const int64_t* matches0, const int32_t* num_keypoints0, float threshold, int32_t hypotheses,
                                int32_t refine, uint64_t seed, int64_t pair_offset, double* H, uint8_t* inliers, int32_t* num_inliers,
                                int32_t* best_model, float* quality, void* workspace_dev, void* stream) {
    og_clear_status();
    if (!quality) return OG_E_INVALID;
    if (m > kSigmaMaxMatches) return OG_E_SHAPE;
    return ransac_run<Homography, 1>(batch, m, n, keypoints0, keypoints1, matches0, num_keypoints0, threshold, hypotheses, refine, seed,
                                     pair_offset, H, inliers, num_inliers, best_model, workspace_dev, stream, quality);
}

extern "C" int og_homography_precision(int32_t batch, int32_t m, int32_t n, const float* keypoints0, const float* keypoints1,
                                       const int64_t* matches0, const int32_t* num_keypoints0, const float* H_true, float threshold,
                                       float* precision, float* matching_score, int32_t* num_correct, void* stream) {
    og_clear_status();
    if (batch <= 0 || m < 0 || n < 0 || !(threshold >= 0.0f) || !precision || !matching_score || !num_correct || !H_true) return OG_E_INVALID;
    if (m > 0 && (!keypoints0 || !matches0 || (n > 0 && !keypoints1))) return OG_E_INVALID;
    const MatchGeo g{keypoints0, keypoints1, matches0, num_keypoints0, batch, m, n};
    hipLaunchKernelGGL(hm_precision_kernel, dim3(batch), dim3(256), 0, (hipStream_t)stream, g, H_true, threshold, precision, matching_score,
                       num_correct);
    return og_launch_status();
}

extern "C" int og_homography_corner_error(int32_t batch, const double* H_est, const float* H_true, int32_t width, int32_t height,
                                          float* error, void* stream) {
    og_clear_status();
    if (batch <= 0 || width <= 0 || height <= 0 || !H_est || !H_true || !error) return OG_E_INVALID;
    hipLaunchKernelGGL(hm_corner_error_kernel, dim3((batch + 63) / 64), dim3(64), 0, (hipStream_t)stream, batch, H_est, H_true, width,
                       height, error);
    return og_launch_status();
}
