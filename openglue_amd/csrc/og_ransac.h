// Helpers every RANSAC unit shares (metrics.hip: five-point / essential matrix; geometry.hip: seven-point / fundamental matrix and
// homography.hip: four-point / homography, both through og_ransac_hartley.h, which includes this file and holds their common skeleton;
// sigma_consensus.hip: the sigma-consensus table on its own): the polynomial helpers, the counter-based draws, the validity rule and
// compaction of matches, the packed winner, sigma-consensus q and w, and jacobi3.
// Internal, not part of the ABI.  Everything lives in the unnamed namespace of the including unit.
// The workgroup sum and the compaction rank come from og_block.h.
#pragma once
#include "og_block.h"
#include "og_sigma_table.h"

namespace {

__host__ __device__ inline bool finite(double v) { return v - v == 0.0; }

template <int NA, int NB>
__host__ __device__ inline void pmul(const double (&a)[NA], const double (&b)[NB], double (&o)[NA + NB - 1]) {
#pragma unroll
    for (int i = 0; i < NA + NB - 1; ++i) o[i] = 0.0;
#pragma unroll
    for (int i = 0; i < NA; ++i)
#pragma unroll
        for (int j = 0; j < NB; ++j) o[i + j] += a[i] * b[j];
}
template <int N>
__host__ __device__ inline double peval(const double* p, double t) {       // ascending coefficients, N of them
    double v = p[N - 1];
#pragma unroll
    for (int i = N - 2; i >= 0; --i) v = v * t + p[i];
    return v;
}

// counter-based hash (splitmix64 finaliser): the RANSAC draws
__host__ __device__ inline uint64_t mix64(uint64_t z) {
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// K distinct positions in [0, n), n >= K, for hypothesis h of pair `pair`: draw j is the hash of (seed, pair, h, j) scaled to n, then
// stepped to the next unused position (at most j steps)
template <int K>
__host__ __device__ inline void draw_distinct(uint64_t seed, uint64_t pair, int h, int n, int (&pick)[K]) {
    const uint64_t base = mix64(mix64(seed) ^ pair) ^ ((uint64_t)h << 8);
#pragma unroll
    for (int j = 0; j < K; ++j) {
        int r = (int)(((mix64(base + j) >> 32) * (uint64_t)n) >> 32);
#pragma unroll
        for (int t = 0; t < K; ++t) {
            bool dup = false;
#pragma unroll
            for (int q = 0; q < j; ++q) dup = dup || pick[q] == r;
            r = dup ? (r + 1 == n ? 0 : r + 1) : r;
        }
        pick[j] = r;
    }
}

// The validity rule of every unit: keypoint i of pair b is matched when i < num_keypoints0[b] and 0 <= matches0[i] < n.  G carries
// matches0 [B][m] int64, nk0 [B] (or null: m), m and n.
template <class G>
__device__ inline bool valid_match(const G& g, int b, int i, int& j) {
    const int lim = g.nk0 ? min(g.nk0[b], g.m) : g.m;
    const int64_t v = g.matches0[(int64_t)b * g.m + i];
    j = (int)v;
    return i < lim && v >= 0 && v < g.n;
}

// One workgroup of 256 compacts the valid matches of pair b in index order into idx (the pair's row, m entries) and returns their
// number in every thread.  each(i, j) runs for every valid match in the thread that found it.  wsum: 4 ints of LDS.  The last
// barrier orders the writes to idx before whatever the workgroup reads from it afterwards.
template <class G, class Each>
__device__ inline int compact_valid_matches(const G& g, int b, int* idx, int* wsum, Each each) {
    int base = 0;
    for (int i0 = 0; i0 < g.m; i0 += 256) {
        const int i = i0 + threadIdx.x;
        int j = 0;
        const bool v = i < g.m && valid_match(g, b, i, j);
        if (v) each(i, j);
        int cnt;
        const int rank = block_rank_of(v, wsum, cnt);
        if (v) idx[base + rank] = i;
        base += cnt;
        __syncthreads();
    }
    return base;
}

__device__ __forceinline__ float4 to_f4(double4 d) { return make_float4((float)d.x, (float)d.y, (float)d.z, (float)d.w); }

// The tail of the score kernels: a thread's key is (inliers + 1) << 32 | ~model, 0 for "no model"; the wave's largest goes into
// the pair's winner by one 64-bit atomicMax (more inliers win, then the lower model index).
__device__ __forceinline__ void publish_best(unsigned long long key, unsigned long long* best) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long other = __shfl_xor(key, o, 64);
        key = other > key ? other : key;
    }
    if ((threadIdx.x & 63) == 0 && key) atomicMax(best, key);
}

// ------------------------------------------------------------------------------------------------ sigma-consensus (MAGSAC++)
// n = 4 degrees of freedom, a = 1.5, k = 3.64, sigma_max = threshold / k.  With t = e / threshold^2 and u = t u_max, u_max = k^2 / 2:
//   w(t) = (G(1.5, u) - G(1.5, u_max)) / (G(1.5) - G(1.5, u_max)),                  G the upper incomplete gamma function,
//   q(t) = 1 - (g(2.5, u) + u (G(1.5, u) - G(1.5, u_max))) / g(2.5, u_max),          g the lower one,
// both 1 at t = 0, 0 at t = 1 and decreasing.  G(1.5, u) = sqrt(u) exp(-u) + (sqrt(pi) / 2) erfc(sqrt u), and with
// g(2.5, u) = 1.5 g(1.5, u) - u^1.5 exp(-u) the numerator of q is 1.5 g(1.5, u) + u ((sqrt(pi) / 2) erfc(sqrt u) - G(1.5, u_max)).
constexpr int kSigmaCells = 1024;                         // the q table: kSigmaCells + 1 floats of LDS
constexpr int kSigmaMaxMatches = 32768;                   // Q + 1 <= 2^31 + 1 fits the upper half of the packed key
constexpr double kSigmaUmax = 6.6248;                     // 3.64^2 / 2
constexpr double kSigmaHalfSqrtPi = 0.88622692545275801;  // G(1.5)
constexpr double kSigmaG1 = 0.0036572608340910764;        // G(1.5, u_max)

// The table (og_sigma_table.h: 65536 q at t = i / kSigmaCells, i = 0 .. kSigmaCells, rounded to fp32 from 40 digits, decreasing from
// 65536 to 0) into LDS by the whole workgroup (256 threads).  The caller puts a barrier before the first sigma_consensus.
__device__ inline void sigma_table_fill(float* tab) {
    for (int i = threadIdx.x; i <= kSigmaCells; i += 256) tab[i] = kSigmaQTable[i];
}

// fp32 t -> (q in units of 2^-16, w); (0, 0) outside [0, 1] and for NaN.  The one function of the score kernels, the finish kernels
// and og_sigma_consensus_eval, so that they agree bitwise.
//  q: the table, linear inside a cell.  t * kSigmaCells, the cell and the fraction are exact in fp32, the FMA is monotone in the
//     fraction and the result never passes the cell's far end, so q does not increase with t: a closed form in fp32 cannot promise
//     that where q is flat (its terms of order 1 cancel to q, leaving 1e-7 of noise on steps smaller than that).  The chord's error is
//     at most q'' h^2 / 8 = 14.5 / 1024^2 / 8 = 1.7e-6, 0.11 units.
//  w: the closed form in fp32 with explicit roundings; at t = 0 numerator and denominator are the same float, so w = 1.
__device__ __forceinline__ void sigma_consensus(const float* tab, float t, uint32_t& q, float& w) {
    const bool in = t >= 0.0f && t <= 1.0f;
    const float tc = in ? t : 1.0f;                         // no branch: outside, the far end is evaluated, where q is 0 by itself
    const float x = __fmul_rn(tc, (float)kSigmaCells);
    const int i = min((int)x, kSigmaCells - 1);
    const float f = x - (float)i;
    const float q0 = tab[i], q1 = tab[i + 1];
    q = (uint32_t)__float2int_rn(fmaxf(__fmaf_rn(f, q1 - q0, q0), q1));      // at tc = 1: fma(1, 0 - q0, q0) = 0
    constexpr float hp = (float)kSigmaHalfSqrtPi, g1 = (float)kSigmaG1;
    const float u = __fmul_rn(tc, (float)kSigmaUmax), s = sqrtf(u);
    const float gu = __fmaf_rn(s, expf(-u), __fmul_rn(hp, erfcf(s)));
    w = in ? fminf(fmaxf(__fdiv_rn(gu - g1, hp - g1), 0.0f), 1.0f) : 0.0f;
}

// 1 / t2 for sigma_match, taken once per kernel; 0 when the bound is 0 (or so small that its reciprocal overflows).
__device__ __forceinline__ float sigma_inv_bound(float t2) {
    const float r = __fdiv_rn(1.0f, t2);
    return r < __builtin_huge_valf() ? r : 0.0f;
}

// A match of squared residual e under the bound t2 (both in the same units; inv_t2 = sigma_inv_bound(t2)): false, q = 0, w = 0 unless
// e <= t2, which covers a NaN or infinite e; otherwise t = min(e * inv_t2, 1), e / t2 to 1.5 ulp without a division per match, and
// t = 0 when the bound is 0.  No branch either: the score loop runs one model per lane, and a branch around the lookup would leave
// each iteration waiting for its own LDS gather.
__device__ __forceinline__ bool sigma_match(const float* tab, float e, float t2, float inv_t2, uint32_t& q, float& w) {
    const bool inl = e <= t2;
    sigma_consensus(tab, inl ? fminf(__fmul_rn(e, inv_t2), 1.0f) : 2.0f, q, w);
    return inl;
}

// the last kernel argument of a sigma-consensus finish kernel is `float* quality`; the hard-count instance has none
__device__ __forceinline__ void store_quality(int, float) {}
__device__ __forceinline__ void store_quality(int b, float v, float* quality) { quality[b] = v; }

// symmetric 3 x 3 eigen-decomposition by cyclic Jacobi: A = V diag(A) V^T on return
__device__ inline void jacobi3(double (&A)[3][3], double (&V)[3][3]) {
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) V[i][j] = i == j ? 1.0 : 0.0;
    for (int sweep = 0; sweep < 12; ++sweep) {
#pragma unroll
        for (int pq = 0; pq < 3; ++pq) {
            const int p = pq == 2 ? 1 : 0, q = pq == 0 ? 1 : 2;
            const double apq = A[p][q];
            if (fabs(apq) < 1e-300) continue;
            const double theta = (A[q][q] - A[p][p]) / (2.0 * apq);
            const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
            const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
            // A <- J^T A J, V <- V J with J_pp = J_qq = c, J_pq = s, J_qp = -s
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const double akp = A[k][p], akq = A[k][q];
                A[k][p] = c * akp - s * akq;
                A[k][q] = s * akp + c * akq;
            }
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const double apk = A[p][k], aqk = A[q][k];
                A[p][k] = c * apk - s * aqk;
                A[q][k] = s * apk + c * aqk;
            }
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const double vkp = V[k][p], vkq = V[k][q];
                V[k][p] = c * vkp - s * vkq;
                V[k][q] = s * vkp + c * vkq;
            }
        }
    }
}

}  // namespace
