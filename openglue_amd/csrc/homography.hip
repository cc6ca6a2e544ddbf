// Planar geometric verification and the validation metrics of the homography pre-training stage: what a user of cv2.findHomography
// gets for a planar scene, for a whole SuperGlue.match batch, without leaving the GPU, and the perspective counterparts of
// og_epipolar_precision / og_relative_pose's error (the reference validates nothing after pretrain_homography.py).
//
//  * og_homography_4pt -- the four-point minimal solver, fp64, one thread per problem:
//      hm_solve_kernel    the 8 x 9 DLT system of the four correspondences (Gauss-Jordan with row pivoting, the free column is the
//                         last), unit Frobenius norm, largest-magnitude entry positive.  A sample yields a model only if every one
//                         of its four point triples has a signed area above 1e-9 in both images with the same sign in both (cv2's
//                         orientation test; it removes collinear triples too), all nine entries are finite and the eight
//                         constraints hold to 1e-9.
//
//  * og_homography -- RANSAC over that solver, then least-squares refits:
//      hm_prep_kernel     hartley_prep_pair (og_ransac.h), exactly what fm_prep_kernel of geometry.hip runs
//      hm_solve_kernel    one thread per (pair, hypothesis): 4 distinct matches drawn by the counter-based hash of og_ransac.h
//      hm_score_kernel    one hypothesis per lane, the pair's points staged through LDS, squared forward transfer error of x0 -> x1
//                         in pixels^2 <= threshold^2 in fp32 on the normalised coordinates (image 1's scale enters the bound); the
//                         winner per pair is a packed 64-bit atomicMax of (inliers + 1, ~hypothesis)
//      hm_finish_kernel   one workgroup per pair: `refine` rounds of {the 45 distinct entries of the 9 x 9 normal matrix of the
//                         inliers' DLT rows (two per match) in fp64 (lanes, then waves), its smallest eigenvector by cyclic Jacobi
//                         with one matrix row per lane, inliers recounted, kept if not fewer}, then the mask by the same fp32 test,
//                         H back in pixels, unit norm, largest entry positive
//    Four launches whatever the batch; no host synchronisation, no float atomics: every output is identical from run to run.
//
//  * og_homography_sc -- the same four launches with sigma-consensus scoring: the score and finish kernels are templates on the
//    scoring mode, this unit instantiates the hard count (SC = 0), and sigma_consensus.hip includes this file with OG_SIGMA_UNIT for
//    the SC = 1 instances and their entry.
//
//  * og_homography_precision -- hm_precision_kernel: per pair, |proj(H_true, k0[i]) - k1[matches0[i]]| in fp64 for every valid match
//  * og_homography_corner_error -- hm_corner_error_kernel: mean distance of the four image corners under the estimate and the truth
#include "og_common.h"
#include "og_ransac.h"

namespace {

constexpr int kHSlots = 9;          // doubles per problem in the H buffer
constexpr int kHChunk = 1024;       // points per LDS stage of the scorer

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

// ------------------------------------------------------------------------------------------------ RANSAC
struct HGeo {
    const float* k0; const float* k1; const int64_t* matches0; const int32_t* nk0;
    int B, m, n;
};

struct HomWs {
    double4* pts;          // [B][m] the valid matches in index order, normalised (u0, v0, u1, v1)
    int* idx;              // [B][m] their keypoint0 index
    int* count;            // [B]
    double* norm;          // [B][6] centroid and scale of image 0, of image 1
    unsigned long long* best;   // [B] packed (inliers + 1, ~hypothesis)
    double* H;             // [B * hypotheses][9]
    int* nsol;             // [B * hypotheses]
};

static size_t hom_bytes(int B, int m, int H) {
    const int64_t bm = (int64_t)B * m, bh = (int64_t)B * H;
    return og_round_up(32 * bm, 256) + og_round_up(4 * bm, 256) + og_round_up(4 * (int64_t)B, 256) + og_round_up(48 * (int64_t)B, 256) +
           og_round_up(8 * (int64_t)B, 256) + og_round_up(8 * kHSlots * bh, 256) + og_round_up(4 * bh, 256);
}

static HomWs hom_layout(void* ws, int B, int m, int H) {
    HomWs w{};
    char* p = (char*)ws;
    const int64_t bm = (int64_t)B * m, bh = (int64_t)B * H;
    auto take = [&](int64_t bytes) { char* r = p; p += og_round_up(bytes, 256); return r; };
    w.pts = (double4*)take(32 * bm);
    w.idx = (int*)take(4 * bm);
    w.count = (int*)take(4 * (int64_t)B);
    w.norm = (double*)take(48 * (int64_t)B);
    w.best = (unsigned long long*)take(8 * (int64_t)B);
    w.H = (double*)take(8 * kHSlots * bh);
    w.nsol = (int*)take(4 * bh);
    return w;
}

__global__ void __launch_bounds__(256) hm_prep_kernel(HGeo g, HomWs w) { hartley_prep_pair(g, w); }

struct HSolveSrc {
    const double* x0; const double* x1;      // direct problems (og_homography_4pt): [count][4][2]
    const double4* pts; const int* cnt;      // RANSAC draws (og_homography): problem = b * H + h
    int m, H;
    uint64_t seed;
    int64_t pair_offset;
};

__global__ void __launch_bounds__(64) hm_solve_kernel(HSolveSrc src, int count, double* Hm, int* nsol) {
    const int p = blockIdx.x * 64 + threadIdx.x;
    if (p >= count) return;
    double x0[8], x1[8];
    if (src.x0) {
#pragma unroll
        for (int i = 0; i < 8; ++i) { x0[i] = src.x0[(int64_t)p * 8 + i]; x1[i] = src.x1[(int64_t)p * 8 + i]; }
    } else {
        const int b = p / src.H, h = p - b * src.H;
        const int n = src.cnt[b];
        if (n < 4) { nsol[p] = 0; return; }
        int pick[4];
        draw_distinct<4>(src.seed, (uint64_t)(src.pair_offset + b), h, n, pick);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const double4 q = src.pts[(int64_t)b * src.m + pick[j]];
            x0[2 * j] = q.x; x0[2 * j + 1] = q.y; x1[2 * j] = q.z; x1[2 * j + 1] = q.w;
        }
    }
    nsol[p] = homography_4pt(x0, x1, Hm + (int64_t)p * kHSlots);
}

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
__device__ __forceinline__ bool transfer_inlier_px(const float (&e)[9], float4 q, float t2s) { return transfer_px(e, q) <= t2s; }

// threshold^2 s1^2 in fp32, the one rounding both kernels use
__device__ __forceinline__ float transfer_bound(float t2, double s1) { return __fmul_rn(t2, (float)(s1 * s1)); }

// SC = 0: a model's score is its number of inliers.  SC = 1: sigma-consensus, the score is Q = sum of q in units of 2^-16 (og_ransac.h).
template <int SC>
__global__ void __launch_bounds__(256) hm_score_kernel(HomWs w, int m, int H, int groups, float t2) {
    __shared__ float4 pts[kHChunk];
    const float* sig = nullptr;
    if constexpr (SC) {
        __shared__ float tab[kSigmaCells + 1];
        sigma_table_fill(tab);                               // the barriers of the first chunk come before its first use
        sig = tab;
    }
    const int b = blockIdx.x / groups;                       // `groups` workgroups per pair, pair-major along x
    const int h = (blockIdx.x - b * groups) * 256 + threadIdx.x;
    const int64_t prob = (int64_t)b * H + h;
    const bool live = h < H && w.nsol[h < H ? prob : 0] > 0;
    float e[9];
#pragma unroll
    for (int c = 0; c < 9; ++c) e[c] = live ? (float)w.H[prob * kHSlots + c] : 0.0f;
    const int n = w.count[b];
    const float t2s = transfer_bound(t2, w.norm[(int64_t)b * 6 + 5]);
    const float inv_t2 = sigma_inv_bound(t2s);               // SC = 1 only
    int inl = 0;
    uint32_t Q = 0u;
    for (int k0 = 0; k0 < n; k0 += kHChunk) {
        const int len = min(kHChunk, n - k0);
        __syncthreads();
        for (int k = threadIdx.x; k < len; k += 256) pts[k] = to_f4(w.pts[(int64_t)b * m + k0 + k]);
        __syncthreads();
        if constexpr (SC) {
            if (live)
#pragma unroll 4
                for (int k = 0; k < len; ++k) {
                    uint32_t q;
                    float wt;
                    sigma_match(sig, transfer_px(e, pts[k]), t2s, inv_t2, q, wt);
                    Q += q;
                }
        } else {
            if (live)
                for (int k = 0; k < len; ++k) inl += transfer_inlier_px(e, pts[k], t2s);      // every lane reads pts[k]: a broadcast
        }
    }
    const unsigned long long score = SC ? (unsigned long long)Q : (unsigned long long)inl;
    const unsigned long long key = live ? ((score + 1) << 32) | (unsigned)(0xFFFFFFFFu - (unsigned)h) : 0ull;
    publish_best(key, &w.best[b]);
}

// SC as in hm_score_kernel.  SC = 1: the refit's rows are weighted by w, a refit is kept if its Q is no smaller, and the last argument
// is `float* quality`, Q / 65536 of the final model.
template <int SC, class... Quality>
__global__ void __launch_bounds__(256) hm_finish_kernel(HGeo g, HomWs w, int H, int refine, float t2, double* H_out, uint8_t* inliers,
                                                        int* num_inliers, int* best_model, Quality... quality) {
    const float* sig = nullptr;
    if constexpr (SC) {
        __shared__ float tab[kSigmaCells + 1];
        sigma_table_fill(tab);
        __syncthreads();
        sig = tab;
    }
    __shared__ double racc[4][45];
    __shared__ double hnew[10];          // the refit and 1.0 if it is sound
    __shared__ int red[4];
    const int b = blockIdx.x, lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int n = w.count[b];
    const unsigned long long key = w.best[b];
    const bool have = key != 0ull && n >= 4;
    const int h = (int)(0xFFFFFFFFu - (unsigned)(key & 0xFFFFFFFFull));
    const double4* P = w.pts + (int64_t)b * g.m;
    for (int i = threadIdx.x; i < g.m; i += 256) inliers[(int64_t)b * g.m + i] = 0;
    if (!have) {
        if (threadIdx.x == 0) {
#pragma unroll
            for (int c = 0; c < 9; ++c) H_out[(int64_t)b * 9 + c] = 0.0;
            num_inliers[b] = 0;
            best_model[b] = -1;
            store_quality(b, 0.0f, quality...);
        }
        return;
    }
    const double s0 = w.norm[(int64_t)b * 6 + 2], s1 = w.norm[(int64_t)b * 6 + 5];
    const float t2s = transfer_bound(t2, s1);
    double Hc[9];
    float e[9];
#pragma unroll
    for (int c = 0; c < 9; ++c) { Hc[c] = w.H[((int64_t)b * H + h) * kHSlots + c]; e[c] = (float)Hc[c]; }
    const float inv_t2 = sigma_inv_bound(t2s);               // SC = 1 only
    auto count_inliers = [&](const float (&f)[9]) {
        int c = 0;
        for (int k = threadIdx.x; k < n; k += 256) c += transfer_inlier_px(f, to_f4(P[k]), t2s);
        return block_sum(c, red);
    };
    // sigma-consensus: the inliers of a model to cnt and its Q returned, one pass
    auto measure = [&](const float (&f)[9], int& cnt) {
        int c = 0;
        uint32_t Q = 0u;
        for (int k = threadIdx.x; k < n; k += 256) {
            uint32_t q;
            float wt;
            c += sigma_match(sig, transfer_px(f, to_f4(P[k])), t2s, inv_t2, q, wt);
            Q += q;
        }
        cnt = block_sum(c, red);
        return block_sum(Q, (uint32_t*)red);
    };
    int cur;
    uint32_t curq = 0u;
    if constexpr (SC) curq = measure(e, cur); else cur = count_inliers(e);
    for (int round = 0; round < refine; ++round) {
        if (cur < 5) break;
        double acc[45];
#pragma unroll
        for (int c = 0; c < 45; ++c) acc[c] = 0.0;
        for (int k = threadIdx.x; k < n; k += 256) {
            const double4 q = P[k];
            uint32_t qk;
            float wt;
            if constexpr (SC) {
                if (!sigma_match(sig, transfer_px(e, to_f4(q)), t2s, inv_t2, qk, wt)) continue;
            } else {
                if (!transfer_inlier_px(e, to_f4(q), t2s)) continue;
            }
            // the two DLT rows of the match: (x0^T, 0, -u1 x0^T) and (0, x0^T, -v1 x0^T)
            const double ra[9] = {q.x, q.y, 1.0, 0.0, 0.0, 0.0, -q.z * q.x, -q.z * q.y, -q.z};
            const double rb[9] = {0.0, 0.0, 0.0, q.x, q.y, 1.0, -q.w * q.x, -q.w * q.y, -q.w};
#pragma unroll
            for (int i = 0; i < 9; ++i) {
                const double ai = SC ? (double)wt * ra[i] : ra[i], bi = SC ? (double)wt * rb[i] : rb[i];      // the weighted rows
#pragma unroll
                for (int j = i; j < 9; ++j) acc[tri(i, j)] += ai * ra[j] + bi * rb[j];
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
            double Hr[9], n2 = 0.0;
#pragma unroll
            for (int k = 0; k < 9; ++k) { Hr[k] = __shfl(col, k, 64); n2 += Hr[k] * Hr[k]; }
            const double inv = 1.0 / sqrt(n2);
            if (lane == 0) {
#pragma unroll
                for (int k = 0; k < 9; ++k) hnew[k] = Hr[k] * inv;
                hnew[9] = finite(inv) ? 1.0 : 0.0;
            }
        }
        __syncthreads();
        double Hn[9];
        float en[9];
#pragma unroll
        for (int c = 0; c < 9; ++c) { Hn[c] = hnew[c]; en[c] = (float)Hn[c]; }
        const bool sound = hnew[9] == 1.0;
        int cnt;                                        // the count's barriers also keep hnew until every lane has read it
        uint32_t qn = 0u;
        if constexpr (SC) qn = measure(en, cnt); else cnt = count_inliers(en);
        if (sound && (SC ? qn >= curq : cnt >= cur)) {
            cur = cnt;
            curq = qn;
#pragma unroll
            for (int c = 0; c < 9; ++c) { Hc[c] = Hn[c]; e[c] = en[c]; }
        }
    }
    __syncthreads();                                    // the zeros above are in memory before the flags
    for (int k = threadIdx.x; k < n; k += 256)
        if (transfer_inlier_px(e, to_f4(P[k]), t2s)) inliers[(int64_t)b * g.m + w.idx[(int64_t)b * g.m + k]] = 1;
    if (threadIdx.x != 0) return;
    // pixels: H = T1^-1 Hn T0 with T = [[s 0 -s cx] [0 s -s cy] [0 0 1]], T^-1 = [[1/s 0 cx] [0 1/s cy] [0 0 1]]
    const double cx0 = w.norm[(int64_t)b * 6 + 0], cy0 = w.norm[(int64_t)b * 6 + 1], cx1 = w.norm[(int64_t)b * 6 + 3], cy1 = w.norm[(int64_t)b * 6 + 4];
    const double is1 = 1.0 / s1;
    double G[9], Hp[9];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        G[r * 3] = s0 * Hc[r * 3];
        G[r * 3 + 1] = s0 * Hc[r * 3 + 1];
        G[r * 3 + 2] = Hc[r * 3 + 2] - s0 * (cx0 * Hc[r * 3] + cy0 * Hc[r * 3 + 1]);
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        Hp[c] = is1 * G[c] + cx1 * G[6 + c];
        Hp[3 + c] = is1 * G[3 + c] + cy1 * G[6 + c];
        Hp[6 + c] = G[6 + c];
    }
    double n2 = 0.0, big = 0.0;
#pragma unroll
    for (int c = 0; c < 9; ++c) { n2 += Hp[c] * Hp[c]; big = fabs(Hp[c]) > fabs(big) ? Hp[c] : big; }
    double inv = 1.0 / sqrt(n2);
    inv = finite(inv) ? (big < 0.0 ? -inv : inv) : 0.0;
#pragma unroll
    for (int c = 0; c < 9; ++c) H_out[(int64_t)b * 9 + c] = Hp[c] * inv;
    num_inliers[b] = cur;
    best_model[b] = h;
    store_quality(b, (float)((double)curq / 65536.0), quality...);
}

#ifndef OG_SIGMA_UNIT
// ------------------------------------------------------------------------------------------------ metrics
// (x, y) under the row-major 3 x 3 Hm, fp64; a point at infinity gives inf or NaN
__device__ inline void project(const double (&Hm)[9], double x, double y, double& u, double& v) {
    const double pw = Hm[6] * x + Hm[7] * y + Hm[8];
    u = (Hm[0] * x + Hm[1] * y + Hm[2]) / pw;
    v = (Hm[3] * x + Hm[4] * y + Hm[5]) / pw;
}

__global__ void __launch_bounds__(256) hm_precision_kernel(HGeo g, const float* H_true, float threshold, float* precision,
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
#endif

}  // namespace

// ------------------------------------------------------------------------------------------------ C ABI
static bool hom_sizes_ok(int32_t batch, int32_t m, int32_t hypotheses) {
    return batch > 0 && m >= 0 && hypotheses > 0 && (int64_t)batch * hypotheses <= (1 << 30);
}

// The four launches of og_homography (SC = 0) and og_homography_sc (SC = 1, quality = one float*).
template <int SC, class... Quality>
static int hom_run(int32_t batch, int32_t m, int32_t n, const float* keypoints0, const float* keypoints1, const int64_t* matches0,
                   const int32_t* num_keypoints0, float threshold, int32_t hypotheses, int32_t refine, uint64_t seed, int64_t pair_offset,
                   double* H, uint8_t* inliers, int32_t* num_inliers, int32_t* best_model, void* workspace_dev, void* stream,
                   Quality... quality) {
    if (!hom_sizes_ok(batch, m, hypotheses) || n < 0 || refine < 0 || !(threshold >= 0.0f) || !H || !num_inliers || !best_model ||
        !workspace_dev)
        return OG_E_INVALID;
    if (m > 0 && (!keypoints0 || !matches0 || !inliers || (n > 0 && !keypoints1))) return OG_E_INVALID;
    if ((uintptr_t)workspace_dev % 16) return OG_E_ALIGN;
    const HGeo g{keypoints0, keypoints1, matches0, num_keypoints0, batch, m, n};
    HomWs w = hom_layout(workspace_dev, batch, m, hypotheses);
    hipStream_t st = (hipStream_t)stream;
    const int count = batch * hypotheses;
    const float t2 = threshold * threshold;
    HSolveSrc src{};
    src.pts = w.pts; src.cnt = w.count; src.m = m; src.H = hypotheses; src.seed = seed; src.pair_offset = pair_offset;
    hipLaunchKernelGGL(hm_prep_kernel, dim3(batch), dim3(256), 0, st, g, w);
    hipLaunchKernelGGL(hm_solve_kernel, dim3((count + 63) / 64), dim3(64), 0, st, src, count, w.H, w.nsol);
    const int groups = (hypotheses + 255) / 256;              // batch * groups <= 2^22 + batch by the size rule: one grid dimension
    hipLaunchKernelGGL(hm_score_kernel<SC>, dim3(batch * groups), dim3(256), 0, st, w, m, hypotheses, groups, t2);
    hipLaunchKernelGGL((hm_finish_kernel<SC, Quality...>), dim3(batch), dim3(256), 0, st, g, w, hypotheses, refine, t2, H, inliers,
                       num_inliers, best_model, quality...);
    return og_launch_status();
}

#ifdef OG_SIGMA_UNIT      // sigma_consensus.hip includes this file for the SC = 1 instances, so that this unit holds the six kernels it held
extern "C" int og_homography_sc(int32_t batch, int32_t m, int32_t n, const float* keypoints0, const float* keypoints1,
                                const int64_t* matches0, const int32_t* num_keypoints0, float threshold, int32_t hypotheses,
                                int32_t refine, uint64_t seed, int64_t pair_offset, double* H, uint8_t* inliers, int32_t* num_inliers,
                                int32_t* best_model, float* quality, void* workspace_dev, void* stream) {
    og_clear_status();
    if (!quality) return OG_E_INVALID;
    if (m > kSigmaMaxMatches) return OG_E_SHAPE;
    return hom_run<1>(batch, m, n, keypoints0, keypoints1, matches0, num_keypoints0, threshold, hypotheses, refine, seed, pair_offset, H,
                      inliers, num_inliers, best_model, workspace_dev, stream, quality);
}
#else
extern "C" int og_homography_4pt(int32_t count, const double* x0, const double* x1, double* H, int32_t* num_solutions, void* stream) {
    og_clear_status();
    if (count <= 0 || count > (1 << 30) || !x0 || !x1 || !H || !num_solutions) return OG_E_INVALID;
    HSolveSrc src{};
    src.x0 = x0; src.x1 = x1;
    hipLaunchKernelGGL(hm_solve_kernel, dim3((count + 63) / 64), dim3(64), 0, (hipStream_t)stream, src, count, H, num_solutions);
    return og_launch_status();
}

extern "C" size_t og_homography_workspace_bytes(int32_t batch, int32_t m, int32_t hypotheses) {
    if (!hom_sizes_ok(batch, m, hypotheses)) return 0;
    return hom_bytes(batch, m, hypotheses);
}

extern "C" int og_homography(int32_t batch, int32_t m, int32_t n, const float* keypoints0, const float* keypoints1,
                             const int64_t* matches0, const int32_t* num_keypoints0, float threshold, int32_t hypotheses,
                             int32_t refine, uint64_t seed, int64_t pair_offset, double* H, uint8_t* inliers, int32_t* num_inliers,
                             int32_t* best_model, void* workspace_dev, void* stream) {
    og_clear_status();
    return hom_run<0>(batch, m, n, keypoints0, keypoints1, matches0, num_keypoints0, threshold, hypotheses, refine, seed, pair_offset, H,
                      inliers, num_inliers, best_model, workspace_dev, stream);
}

extern "C" int og_homography_precision(int32_t batch, int32_t m, int32_t n, const float* keypoints0, const float* keypoints1,
                                       const int64_t* matches0, const int32_t* num_keypoints0, const float* H_true, float threshold,
                                       float* precision, float* matching_score, int32_t* num_correct, void* stream) {
    og_clear_status();
    if (batch <= 0 || m < 0 || n < 0 || !(threshold >= 0.0f) || !precision || !matching_score || !num_correct || !H_true) return OG_E_INVALID;
    if (m > 0 && (!keypoints0 || !matches0 || (n > 0 && !keypoints1))) return OG_E_INVALID;
    const HGeo g{keypoints0, keypoints1, matches0, num_keypoints0, batch, m, n};
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
#endif
