// The RANSAC skeleton of the Hartley-normalised estimators (geometry.hip: Fundamental, homography.hip: Homography): the workspace, the
// four kernels and their launches, written once over a model struct M.  Internal, not part of the ABI; everything lives in the unnamed
// namespace of the including unit.  metrics.hip's calibrated five-point path has its own kernels and includes og_ransac.h alone.
//
//      ransac_prep_kernel<M>      one workgroup per pair: the valid matches compacted in index order, Hartley normalisation of both
//                                 images (centroid, mean distance sqrt 2) in fp64, summed over the COMPACTED order lanes-then-waves, so
//                                 that a pair gives the same bits whatever holes or padding surround its matches
//      ransac_solve_kernel<M>     one thread per (pair, hypothesis): M::kSample distinct matches drawn by the counter-based hash of
//                                 og_ransac.h, or one thread per direct problem (minimal_solve), through M::solve
//      ransac_score_kernel<M, SC> one model (hypothesis, solution) per lane, the pair's points staged through LDS, M::error in fp32 on
//                                 the normalised coordinates against the pair's bound; the winner per pair is a packed 64-bit
//                                 atomicMax of (score + 1, ~model index)
//      ransac_finish_kernel<M, SC, Quality...>
//                                 one workgroup per pair: `refine` rounds of {the 45 distinct entries of the 9 x 9 normal matrix of
//                                 M::rows / M::term over the inliers in fp64 (lanes, then waves), its smallest eigenvector by cyclic
//                                 Jacobi with one matrix row per lane, M::polish, the score taken again, kept if not worse}, then the mask by the
//                                 same fp32 test, the model back in pixels (M::to_pixels), unit norm, largest entry positive
//    ransac_run<M, SC> checks the arguments and makes the four launches whatever the batch; no host synchronisation, no float atomics:
//    every output is identical from run to run.  SC = 0: a model's score is its number of inliers.  SC = 1: sigma-consensus, the score
//    is Q = sum of q in units of 2^-16 (og_ransac.h), the refit's rows are weighted by w, a refit is kept if its Q is no smaller, and the
//    last kernel argument is `float* quality`, Q / 65536 of the final model.
//
// A model struct supplies, all static:
//      kSample, kSol, kSlots      matches per sample, models per sample, doubles per problem in the model buffer (kSol * 9)
//      solve(x0, x1, out)         the minimal solver: [kSample][2] coordinates of order 1 -> up to kSol row-major models, their count
//      Pair, pair(t2, s0, s1)     the per-pair fp32 constants of the error test from threshold^2 and the two scales; Pair::bound is
//                                 what the error is compared with
//      error(e, q, pair)          the fp32 squared error of match q = (u0, v0, u1, v1) under model e
//      Rows, rows(q)              the match's constraint rows, by value (with a hook that adds into the 45 accumulators through a
//                                 reference the compiler made 28 selects of the keep-if-not-worse branch in the SC = 0 finish kernels)
//      term<SC>(rows, wt, i, j)   what the rows, weighted by wt if SC, add to entry (i, j) of the normal matrix
//      polish(v)                  the eigenvector made a model at unit Frobenius norm; false if it is not sound
//      to_pixels(G, s1, cx1, cy1, out)   G = (model) T0 taken through image 1's normalisation
#pragma once
#include "og_ransac.h"

namespace {

constexpr int kRansacChunk = 1024;      // points per LDS stage of the scorer

struct MatchGeo {
    const float* k0; const float* k1; const int64_t* matches0; const int32_t* nk0;
    int B, m, n;
};

struct RansacWs {
    double4* pts;          // [B][m] the valid matches in index order, normalised (u0, v0, u1, v1)
    int* idx;              // [B][m] their keypoint0 index
    int* count;            // [B]
    double* norm;          // [B][6] centroid and scale of image 0, of image 1
    unsigned long long* best;   // [B] packed (score + 1, ~model)
    double* model;         // [B * H][M::kSlots]
    int* nsol;             // [B * H]
};

template <class M>
bool ransac_sizes_ok(int32_t batch, int32_t m, int32_t hypotheses) {
    return batch > 0 && m >= 0 && hypotheses > 0 && (int64_t)M::kSol * batch * hypotheses <= (1 << 30);
}

template <class M>
size_t ransac_bytes(int B, int m, int H) {
    const int64_t bm = (int64_t)B * m, bh = (int64_t)B * H;
    return og_round_up(32 * bm, 256) + og_round_up(4 * bm, 256) + og_round_up(4 * (int64_t)B, 256) + og_round_up(48 * (int64_t)B, 256) +
           og_round_up(8 * (int64_t)B, 256) + og_round_up(8 * M::kSlots * bh, 256) + og_round_up(4 * bh, 256);
}

template <class M>
RansacWs ransac_layout(void* ws, int B, int m, int H) {
    RansacWs w{};
    char* p = (char*)ws;
    const int64_t bm = (int64_t)B * m, bh = (int64_t)B * H;
    auto take = [&](int64_t bytes) { char* r = p; p += og_round_up(bytes, 256); return r; };
    w.pts = (double4*)take(32 * bm);
    w.idx = (int*)take(4 * bm);
    w.count = (int*)take(4 * (int64_t)B);
    w.norm = (double*)take(48 * (int64_t)B);
    w.best = (unsigned long long*)take(8 * (int64_t)B);
    w.model = (double*)take(8 * M::kSlots * bh);
    w.nsol = (int*)take(4 * bh);
    return w;
}

// One workgroup of 256 per pair: the valid matches compacted in index order, both images normalised in fp64 (centroid, mean distance
// sqrt 2) with every sum over the COMPACTED order lanes-then-waves, and the pair's winner reset.  W carries pts [B][m] double4
// (u0, v0, u1, v1), idx [B][m], count [B], norm [B][6] (centroid and scale of image 0, of image 1) and best [B].
template <class G, class W>
__device__ inline void hartley_prep_pair(const G& g, const W& w) {
    __shared__ int wsum[4];
    __shared__ double red[4];
    const int b = blockIdx.x;
    const int n = compact_valid_matches(g, b, w.idx + (int64_t)b * g.m, wsum, [](int, int) {});      // the rule and order of metrics.hip
    // pixel coordinates of compacted match k (idx was written by this workgroup before the last barrier of the compaction)
    auto pixel = [&](int k) {
        const int i = w.idx[(int64_t)b * g.m + k];
        const int j = (int)g.matches0[(int64_t)b * g.m + i];
        const float2 a = ((const float2*)g.k0)[(int64_t)b * g.m + i];
        const float2 c = ((const float2*)g.k1)[(int64_t)b * g.n + j];
        return make_double4((double)a.x, (double)a.y, (double)c.x, (double)c.y);
    };
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    for (int k = threadIdx.x; k < n; k += 256) {
        const double4 q = pixel(k);
        s[0] += q.x; s[1] += q.y; s[2] += q.z; s[3] += q.w;
    }
    const double inv_n = n > 0 ? 1.0 / (double)n : 0.0;
    double cen[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) cen[c] = block_sum(s[c], red) * inv_n;
    double d[2] = {0.0, 0.0};
    for (int k = threadIdx.x; k < n; k += 256) {
        const double4 q = pixel(k);
        d[0] += sqrt((q.x - cen[0]) * (q.x - cen[0]) + (q.y - cen[1]) * (q.y - cen[1]));
        d[1] += sqrt((q.z - cen[2]) * (q.z - cen[2]) + (q.w - cen[3]) * (q.w - cen[3]));
    }
    double sc[2];
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        const double mean = block_sum(d[c], red) * inv_n;
        const double v = M_SQRT2 / mean;
        sc[c] = (mean > 0.0 && finite(v)) ? v : 1.0;              // every point on the centroid: leave the scale alone
    }
    for (int k = threadIdx.x; k < n; k += 256) {
        const double4 q = pixel(k);
        w.pts[(int64_t)b * g.m + k] = make_double4(sc[0] * (q.x - cen[0]), sc[0] * (q.y - cen[1]), sc[1] * (q.z - cen[2]), sc[1] * (q.w - cen[3]));
    }
    if (threadIdx.x == 0) {
        double* o = w.norm + (int64_t)b * 6;
        o[0] = cen[0]; o[1] = cen[1]; o[2] = sc[0]; o[3] = cen[2]; o[4] = cen[3]; o[5] = sc[1];
        w.count[b] = n;
        w.best[b] = 0ull;
    }
}

// index of (i, j) among the 45 distinct entries of a symmetric 9 x 9 matrix, rows of the upper triangle one after the other
__host__ __device__ constexpr int tri(int i, int j) { return i <= j ? i * 9 - i * (i - 1) / 2 + (j - i) : j * 9 - j * (j - 1) / 2 + (i - j); }

// Symmetric 9 x 9 eigen-decomposition by cyclic Jacobi, the form of jacobi3 spread over one wave: lane k < 9 holds row k of A (a) and
// row k of V (v); the other lanes carry zeros along.  A rotation (p, q) updates columns p, q of A and V inside every lane, and rows
// p, q of A in the lanes p and q, which read each other's row.  All 64 lanes must call it.  On return a[k] of lane k is eigenvalue k
// and column k of V its eigenvector.
__device__ inline void jacobi9_wave(double (&a)[9], double (&v)[9], int lane) {
#pragma unroll
    for (int j = 0; j < 9; ++j) v[j] = lane == j ? 1.0 : 0.0;
    for (int sweep = 0; sweep < 16; ++sweep) {
        double off = 0.0, dia = 0.0;
#pragma unroll
        for (int j = 0; j < 9; ++j) { off += lane == j ? 0.0 : a[j] * a[j]; dia += lane == j ? a[j] * a[j] : 0.0; }
#pragma unroll
        for (int o = 8; o > 0; o >>= 1) { off += __shfl_xor(off, o, 64); dia += __shfl_xor(dia, o, 64); }
        off = __shfl(off, 0, 64); dia = __shfl(dia, 0, 64);
        if (!(off > 1e-34 * dia)) break;
#pragma unroll
        for (int p = 0; p < 8; ++p)
#pragma unroll
            for (int q = p + 1; q < 9; ++q) {
                const double app = __shfl(a[p], p, 64), aqq = __shfl(a[q], q, 64), apq = __shfl(a[q], p, 64);
                const bool rot = fabs(apq) >= 1e-300;
                const double theta = (aqq - app) / (2.0 * (rot ? apq : 1.0));
                const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                const double c = rot ? 1.0 / sqrt(t * t + 1.0) : 1.0, s = rot ? t * c : 0.0;
                // A <- J^T A J, V <- V J with J_pp = J_qq = c, J_pq = s, J_qp = -s
                const double akp = a[p], akq = a[q];
                a[p] = c * akp - s * akq;
                a[q] = s * akp + c * akq;
#pragma unroll
                for (int k = 0; k < 9; ++k) {
                    const double apk = __shfl(a[k], p, 64), aqk = __shfl(a[k], q, 64);
                    a[k] = lane == p ? c * apk - s * aqk : lane == q ? s * apk + c * aqk : a[k];
                }
                const double vkp = v[p], vkq = v[q];
                v[p] = c * vkp - s * vkq;
                v[q] = s * vkp + c * vkq;
            }
    }
}

// the hard test of a match under model e, the one form of the score and finish kernels
template <class M>
__device__ __forceinline__ bool ransac_inlier(const float (&e)[9], float4 q, const typename M::Pair& pc) { return M::error(e, q, pc) <= pc.bound; }

template <class M>
__global__ void __launch_bounds__(256) ransac_prep_kernel(MatchGeo g, RansacWs w) { hartley_prep_pair(g, w); }

struct SolveSrc {
    const double* x0; const double* x1;      // direct problems (minimal_solve): [count][M::kSample][2]
    const double4* pts; const int* cnt;      // RANSAC draws (ransac_run): problem = b * H + h
    int m, H;
    uint64_t seed;
    int64_t pair_offset;
};

template <class M>
__global__ void __launch_bounds__(64) ransac_solve_kernel(SolveSrc src, int count, double* model, int* nsol) {
    constexpr int K = M::kSample;
    const int p = blockIdx.x * 64 + threadIdx.x;
    if (p >= count) return;
    double x0[2 * K], x1[2 * K];
    if (src.x0) {
#pragma unroll
        for (int i = 0; i < 2 * K; ++i) { x0[i] = src.x0[(int64_t)p * (2 * K) + i]; x1[i] = src.x1[(int64_t)p * (2 * K) + i]; }
    } else {
        const int b = p / src.H, h = p - b * src.H;
        const int n = src.cnt[b];
        if (n < K) { nsol[p] = 0; return; }
        int pick[K];
        draw_distinct<K>(src.seed, (uint64_t)(src.pair_offset + b), h, n, pick);
#pragma unroll
        for (int j = 0; j < K; ++j) {
            const double4 q = src.pts[(int64_t)b * src.m + pick[j]];
            x0[2 * j] = q.x; x0[2 * j + 1] = q.y; x1[2 * j] = q.z; x1[2 * j + 1] = q.w;
        }
    }
    nsol[p] = M::solve(x0, x1, model + (int64_t)p * M::kSlots);
}

template <class M, int SC>
__global__ void __launch_bounds__(256) ransac_score_kernel(RansacWs w, int m, int H, int groups, float t2) {
    __shared__ float4 pts[kRansacChunk];
    const float* sig = nullptr;
    if constexpr (SC) {
        __shared__ float tab[kSigmaCells + 1];
        sigma_table_fill(tab);                               // the barriers of the first chunk come before its first use
        sig = tab;
    }
    const int b = blockIdx.x / groups;                       // `groups` workgroups per pair, pair-major along x
    const int model = (blockIdx.x - b * groups) * 256 + threadIdx.x;        // h * kSol + s
    const int h = model / M::kSol, s = model - h * M::kSol;
    const int64_t prob = (int64_t)b * H + h;
    const bool live = h < H && s < w.nsol[h < H ? prob : 0];
    float e[9];
#pragma unroll
    for (int c = 0; c < 9; ++c) e[c] = live ? (float)w.model[prob * M::kSlots + s * 9 + c] : 0.0f;
    const int n = w.count[b];
    const typename M::Pair pc = M::pair(t2, w.norm[(int64_t)b * 6 + 2], w.norm[(int64_t)b * 6 + 5]);
    const float inv_t2 = sigma_inv_bound(pc.bound);          // SC = 1 only
    int inl = 0;
    uint32_t Q = 0u;
    for (int k0 = 0; k0 < n; k0 += kRansacChunk) {
        const int len = min(kRansacChunk, n - k0);
        __syncthreads();
        for (int k = threadIdx.x; k < len; k += 256) pts[k] = to_f4(w.pts[(int64_t)b * m + k0 + k]);
        __syncthreads();
        if constexpr (SC) {
            if (live)
#pragma unroll 4
                for (int k = 0; k < len; ++k) {
                    uint32_t q;
                    float wt;
                    sigma_match(sig, M::error(e, pts[k], pc), pc.bound, inv_t2, q, wt);
                    Q += q;
                }
        } else {
            if (live)
                for (int k = 0; k < len; ++k) inl += ransac_inlier<M>(e, pts[k], pc);      // every lane reads pts[k]: a broadcast
        }
    }
    const unsigned long long score = SC ? (unsigned long long)Q : (unsigned long long)inl;
    const unsigned long long key = live ? ((score + 1) << 32) | (unsigned)(0xFFFFFFFFu - (unsigned)model) : 0ull;
    publish_best(key, &w.best[b]);
}

template <class M, int SC, class... Quality>
__global__ void __launch_bounds__(256) ransac_finish_kernel(MatchGeo g, RansacWs w, int H, int refine, float t2, double* out,
                                                            uint8_t* inliers, int* num_inliers, int* best_model, Quality... quality) {
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
    const bool have = key != 0ull && n >= M::kSample;
    const int model = (int)(0xFFFFFFFFu - (unsigned)(key & 0xFFFFFFFFull));
    const int h = model / M::kSol, s = model - h * M::kSol;
    const double4* P = w.pts + (int64_t)b * g.m;
    for (int i = threadIdx.x; i < g.m; i += 256) inliers[(int64_t)b * g.m + i] = 0;
    if (!have) {
        if (threadIdx.x == 0) {
#pragma unroll
            for (int c = 0; c < 9; ++c) out[(int64_t)b * 9 + c] = 0.0;
            num_inliers[b] = 0;
            best_model[b] = -1;
            store_quality(b, 0.0f, quality...);
        }
        return;
    }
    const double s0 = w.norm[(int64_t)b * 6 + 2], s1 = w.norm[(int64_t)b * 6 + 5];
    const typename M::Pair pc = M::pair(t2, s0, s1);
    double Fc[9];
    float e[9];
#pragma unroll
    for (int c = 0; c < 9; ++c) { Fc[c] = w.model[((int64_t)b * H + h) * M::kSlots + s * 9 + c]; e[c] = (float)Fc[c]; }
    const float inv_t2 = sigma_inv_bound(pc.bound);          // SC = 1 only
    auto count_inliers = [&](const float (&f)[9]) {
        int c = 0;
        for (int k = threadIdx.x; k < n; k += 256) c += ransac_inlier<M>(f, to_f4(P[k]), pc);
        return block_sum(c, red);
    };
    // sigma-consensus: the inliers of a model to cnt and its Q returned, one pass
    auto measure = [&](const float (&f)[9], int& cnt) {
        int c = 0;
        uint32_t Q = 0u;
        for (int k = threadIdx.x; k < n; k += 256) {
            uint32_t q;
            float wt;
            c += sigma_match(sig, M::error(f, to_f4(P[k]), pc), pc.bound, inv_t2, q, wt);
            Q += q;
        }
        cnt = block_sum(c, red);
        return block_sum(Q, (uint32_t*)red);
    };
    int cur;
    uint32_t curq = 0u;
    if constexpr (SC) curq = measure(e, cur); else cur = count_inliers(e);
    for (int round = 0; round < refine; ++round) {
        if (cur < M::kSample + 1) break;
        double acc[45];
#pragma unroll
        for (int c = 0; c < 45; ++c) acc[c] = 0.0;
        for (int k = threadIdx.x; k < n; k += 256) {
            const double4 q = P[k];
            uint32_t qk;
            float wt = 1.0f;                            // SC = 0: every inlier weighs the same, and term<0> does not read it
            if constexpr (SC) {
                if (!sigma_match(sig, M::error(e, to_f4(q), pc), pc.bound, inv_t2, qk, wt)) continue;
            } else {
                if (!ransac_inlier<M>(e, to_f4(q), pc)) continue;
            }
            const typename M::Rows r = M::rows(q);
#pragma unroll
            for (int i = 0; i < 9; ++i) {
#pragma unroll
                for (int j = i; j < 9; ++j) acc[tri(i, j)] += M::template term<SC>(r, wt, i, j);
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
            const bool sound = M::polish(Fr);
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
        if (ransac_inlier<M>(e, to_f4(P[k]), pc)) inliers[(int64_t)b * g.m + w.idx[(int64_t)b * g.m + k]] = 1;
    if (threadIdx.x != 0) return;
    // pixels: G = Fc T0 with T = [[s 0 -s cx] [0 s -s cy] [0 0 1]], then image 1's side by the model
    const double cx0 = w.norm[(int64_t)b * 6 + 0], cy0 = w.norm[(int64_t)b * 6 + 1], cx1 = w.norm[(int64_t)b * 6 + 3], cy1 = w.norm[(int64_t)b * 6 + 4];
    double G[9], Fp[9];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        G[r * 3] = s0 * Fc[r * 3];
        G[r * 3 + 1] = s0 * Fc[r * 3 + 1];
        G[r * 3 + 2] = Fc[r * 3 + 2] - s0 * (cx0 * Fc[r * 3] + cy0 * Fc[r * 3 + 1]);
    }
    M::to_pixels(G, s1, cx1, cy1, Fp);
    double n2 = 0.0, big = 0.0;
#pragma unroll
    for (int c = 0; c < 9; ++c) { n2 += Fp[c] * Fp[c]; big = fabs(Fp[c]) > fabs(big) ? Fp[c] : big; }
    double inv = 1.0 / sqrt(n2);
    inv = finite(inv) ? (big < 0.0 ? -inv : inv) : 0.0;
#pragma unroll
    for (int c = 0; c < 9; ++c) out[(int64_t)b * 9 + c] = Fp[c] * inv;
    num_inliers[b] = cur;
    best_model[b] = model;
    store_quality(b, (float)((double)curq / 65536.0), quality...);
}

// The minimal solver on `count` direct problems: og_fundamental_7pt, og_homography_4pt.
template <class M>
int minimal_solve(int32_t count, const double* x0, const double* x1, double* model, int32_t* num_solutions, void* stream) {
    if (count <= 0 || count > (1 << 30) || !x0 || !x1 || !model || !num_solutions) return OG_E_INVALID;
    SolveSrc src{};
    src.x0 = x0; src.x1 = x1;
    hipLaunchKernelGGL(ransac_solve_kernel<M>, dim3((count + 63) / 64), dim3(64), 0, (hipStream_t)stream, src, count, model, num_solutions);
    return og_launch_status();
}

// The four launches of a plain entry (SC = 0) and of its sigma-consensus entry (SC = 1, quality = one float*).
template <class M, int SC, class... Quality>
int ransac_run(int32_t batch, int32_t m, int32_t n, const float* keypoints0, const float* keypoints1, const int64_t* matches0,
               const int32_t* num_keypoints0, float threshold, int32_t hypotheses, int32_t refine, uint64_t seed, int64_t pair_offset,
               double* out, uint8_t* inliers, int32_t* num_inliers, int32_t* best_model, void* workspace_dev, void* stream,
               Quality... quality) {
    if (!ransac_sizes_ok<M>(batch, m, hypotheses) || n < 0 || refine < 0 || !(threshold >= 0.0f) || !out || !num_inliers || !best_model ||
        !workspace_dev)
        return OG_E_INVALID;
    if (m > 0 && (!keypoints0 || !matches0 || !inliers || (n > 0 && !keypoints1))) return OG_E_INVALID;
    if ((uintptr_t)workspace_dev % 16) return OG_E_ALIGN;
    const MatchGeo g{keypoints0, keypoints1, matches0, num_keypoints0, batch, m, n};
    RansacWs w = ransac_layout<M>(workspace_dev, batch, m, hypotheses);
    hipStream_t st = (hipStream_t)stream;
    const int count = batch * hypotheses;
    const float t2 = threshold * threshold;
    SolveSrc src{};
    src.pts = w.pts; src.cnt = w.count; src.m = m; src.H = hypotheses; src.seed = seed; src.pair_offset = pair_offset;
    hipLaunchKernelGGL(ransac_prep_kernel<M>, dim3(batch), dim3(256), 0, st, g, w);
    hipLaunchKernelGGL(ransac_solve_kernel<M>, dim3((count + 63) / 64), dim3(64), 0, st, src, count, w.model, w.nsol);
    const int groups = (hypotheses * M::kSol + 255) / 256;    // batch * groups <= 2^22 + batch by the size rule: one grid dimension
    hipLaunchKernelGGL((ransac_score_kernel<M, SC>), dim3(batch * groups), dim3(256), 0, st, w, m, hypotheses, groups, t2);
    hipLaunchKernelGGL((ransac_finish_kernel<M, SC, Quality...>), dim3(batch), dim3(256), 0, st, g, w, hypotheses, refine, t2, out, inliers,
                       num_inliers, best_model, quality...);
    return og_launch_status();
}

}  // namespace
