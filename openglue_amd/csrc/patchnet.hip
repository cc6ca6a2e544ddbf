// DoG + AffNet + OriNet + HardNet, the part after the detector (reference models/features/opencv/dog_affnet_harnet.py, a kornia
// 0.6-era reading; tests/patchnet_ref.py is the float64 specification).  Inference only, exact fp32 throughout, no float atomics:
// every output is bit-identical from run to run.
//
//   pyramid      level 0 = the image; level l + 1 = level l blurred with [1 4 6 4 1]^2 / 256 (reflect, no edge repeat), then resized
//                bilinearly (align_corners = False) to (floor(h / 2), floor(w / 2)); built while min(h, w) >= 32.
//   extract      one workgroup per LAF: level max(0, floor(log2(2 scale / 32))) of the level-0 LAF (a level that was not built gives
//                zeros), bilinear sampling with border clamping, optionally (x - mean) / (std + 1e-6) with the unbiased std.
//   conv0        1 -> C1 (3x3, pad 1) on the VALU, one workgroup per patch, with the input normalisation when the patches are raw.
//   conv3x3      implicit GEMM on v_mfma_f32_32x32x2_f32.  A workgroup owns 128 output pixels x all output channels: 4 rows of a
//                32 x 32 map, 8 rows of a 16 x 16 map, or two whole 8 x 8 maps; wave w owns pixels 32 w .. 32 w + 31 (whole rows of
//                ONE patch) and Cout / 32 accumulator tiles.  The input rows with their halo are staged in LDS KC channels at a time,
//                a pixel outside its own patch is zero (never the neighbouring patch); the K loop runs over 9 taps x KC channels
//                reading A fragments at tap offsets, stride 1 or 2.  Weights are fragment-major (pack_fragments of og_conv_f32.h, shared with
//                superpoint.hip) with BatchNorm folded; ReLU in the
//                epilogue.  Cout = 16 runs as a 32-wide tile whose upper half is zero weights.
//   tail         the 8 x 8 convolution is a [n, 64 C] x [64 C, Cout] product.  HardNet: MFMA, a workgroup owns 32 patches x 32
//                channels, its 4 waves a quarter of K each, summed in LDS in wave order; then BN(20) as a bias and a row L2
//                normalisation.  AffNet / OriNet (3 / 2 outputs): one wave per patch, VALU, then bias, tanh and the LAF update.
#include "og_conv_f32.h"
#include <cmath>

namespace {

constexpr int PN_PS = 32;
constexpr int PN_MAX_LEVELS = 12;
constexpr int PN_CHUNK = 512;                        // patches per pass through the trunk (bounds the activation buffers)
constexpr int PN_HARDNET = 0, PN_AFFNET = 1, PN_ORINET = 2;

struct PnLevels {
    int levels;
    int h[PN_MAX_LEVELS], w[PN_MAX_LEVELS];
    int64_t off[PN_MAX_LEVELS];                      // per image: floats before level l; level l of a batch starts at B * off[l]
    int64_t floats;                                  // per image
};
PnLevels pn_levels(int H, int W) {
    PnLevels g{};
    int h = H, w = W;
    int64_t o = 0;
    while ((h < w ? h : w) >= PN_PS && g.levels < PN_MAX_LEVELS) {
        g.h[g.levels] = h;
        g.w[g.levels] = w;
        g.off[g.levels] = o;
        o += (int64_t)h * w;
        ++g.levels;
        h /= 2;
        w /= 2;
    }
    g.floats = o;
    return g;
}
bool pn_image_ok(int B, int H, int W) { return B >= 1 && H >= 1 && W >= 1 && H <= 8192 && W <= 8192 && (int64_t)B * H * W <= (1ll << 22); }

// ---------------------------------------------------------------- pyramid
__device__ __forceinline__ int pn_reflect(int i, int n) { return i < 0 ? -i : (i >= n ? 2 * n - 2 - i : i); }

__global__ __launch_bounds__(256) void pn_blur_kernel(const float* __restrict__ in, int B, int h, int w, float* __restrict__ out) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= (int64_t)B * h * w) return;
    const int x = (int)(t % w), y = (int)((t / w) % h);
    const float* im = in + (t / ((int64_t)w * h)) * h * w;
    const float k[5] = {1.f, 4.f, 6.f, 4.f, 1.f};
    float acc = 0.f;
#pragma unroll
    for (int dy = 0; dy < 5; ++dy) {
        const float* row = im + (int64_t)pn_reflect(y + dy - 2, h) * w;
        float r = 0.f;
#pragma unroll
        for (int dx = 0; dx < 5; ++dx) r = fmaf(k[dx], row[pn_reflect(x + dx - 2, w)], r);
        acc = fmaf(k[dy], r, acc);
    }
    out[t] = acc * (1.f / 256.f);
}

// F.interpolate(mode="bilinear", align_corners=False): src = scale (dst + 0.5) - 0.5 clamped at 0, index clamped at size - 1
__global__ __launch_bounds__(256) void pn_resize_kernel(const float* __restrict__ in, int B, int h, int w, int ho, int wo, float* __restrict__ out) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= (int64_t)B * ho * wo) return;
    const int x = (int)(t % wo), y = (int)((t / wo) % ho);
    const float* im = in + (t / ((int64_t)wo * ho)) * h * w;
    const float sy = fmaxf(((float)h / (float)ho) * ((float)y + 0.5f) - 0.5f, 0.f);
    const float sx = fmaxf(((float)w / (float)wo) * ((float)x + 0.5f) - 0.5f, 0.f);
    const int y0 = min((int)sy, h - 1), x0 = min((int)sx, w - 1);
    const int y1 = min(y0 + 1, h - 1), x1 = min(x0 + 1, w - 1);
    const float ly = fminf(fmaxf(sy - (float)y0, 0.f), 1.f), lx = fminf(fmaxf(sx - (float)x0, 0.f), 1.f);
    const float top = (1.f - lx) * im[(int64_t)y0 * w + x0] + lx * im[(int64_t)y0 * w + x1];
    const float bot = (1.f - lx) * im[(int64_t)y1 * w + x0] + lx * im[(int64_t)y1 * w + x1];
    out[t] = (1.f - ly) * top + ly * bot;
}

// ---------------------------------------------------------------- per-patch normalisation: 256 threads x 4 pixels
// (x - mean) / (std + 1e-6), unbiased std over the 1024 pixels; sums in a fixed order (wave butterfly, then waves 0..3)
__device__ __forceinline__ void pn_normalize4(f32x4& v, float* red /* shared [8] */) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float s = wave_sum((v[0] + v[1]) + (v[2] + v[3]));
    if (lane == 0) red[wave] = s;
    __syncthreads();
    const float mean = ((red[0] + red[1]) + (red[2] + red[3])) * (1.f / 1024.f);
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] -= mean;
    const float q = wave_sum((v[0] * v[0] + v[1] * v[1]) + (v[2] * v[2] + v[3] * v[3]));
    if (lane == 0) red[4 + wave] = q;
    __syncthreads();
    const float sd = sqrtf(((red[4] + red[5]) + (red[6] + red[7])) * (1.f / 1023.f));
    const float d = sd + 1e-6f;
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = v[e] / d;
}

// ---------------------------------------------------------------- extract: one workgroup per LAF
__global__ __launch_bounds__(256) void pn_extract_kernel(const float* __restrict__ pyr, PnLevels g, int B, int n, const float* __restrict__ lafs,
                                                         int upright, int normalize, float* __restrict__ patches) {
    __shared__ float red[8];
    const int64_t p = blockIdx.x;
    const int b = (int)(p / n), tid = threadIdx.x;
    const float* L = lafs + p * 6;
    float a00 = L[0], a01 = L[1], a10 = L[3], a11 = L[4];
    const float cx = L[2], cy = L[5];
    const float sc = sqrtf(fabsf(a00 * a11 - a01 * a10));
    if (upright) {
        a00 = sc; a01 = 0.f; a10 = 0.f; a11 = sc;
    }
    int lev = 0;                                       // max(0, floor(log2(2 sc / 32))) by exact halvings
    for (float t = sc * (1.f / 16.f); t >= 2.f && lev < PN_MAX_LEVELS; t *= 0.5f) ++lev;
    f32x4 v{0.f, 0.f, 0.f, 0.f};
    if (lev < g.levels) {
        const int hl = g.h[lev], wl = g.w[lev];
        const float* im = pyr + (int64_t)B * g.off[lev] + (int64_t)b * hl * wl;
        const float r = (float)(min(hl, wl) - 1) / (float)(min(g.h[0], g.w[0]) - 1);
        a00 *= r; a01 *= r; a10 *= r; a11 *= r;
        const float cxl = cx * (float)(wl - 1) / (float)(g.w[0] - 1) - 0.5f;
        const float cyl = cy * (float)(hl - 1) / (float)(g.h[0] - 1) - 0.5f;
        const int i = tid >> 3;
        const float gy = (float)(2 * i + 1) * (1.f / PN_PS) - 1.f;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int j = (tid & 7) * 4 + e;
            const float gx = (float)(2 * j + 1) * (1.f / PN_PS) - 1.f;
            const float x = fminf(fmaxf(a00 * gx + a01 * gy + cxl, 0.f), (float)(wl - 1));      // padding_mode="border"
            const float y = fminf(fmaxf(a10 * gx + a11 * gy + cyl, 0.f), (float)(hl - 1));
            const float fx = floorf(x), fy = floorf(y);
            const int x0 = (int)fx, y0 = (int)fy;
            const int x1 = min(x0 + 1, wl - 1), y1 = min(y0 + 1, hl - 1);
            const float lx = x - fx, ly = y - fy;
            const float v00 = im[(int64_t)y0 * wl + x0], v01 = im[(int64_t)y0 * wl + x1];
            const float v10 = im[(int64_t)y1 * wl + x0], v11 = im[(int64_t)y1 * wl + x1];
            v[e] = (1.f - lx) * (1.f - ly) * v00 + lx * (1.f - ly) * v01 + (1.f - lx) * ly * v10 + lx * ly * v11;
        }
    }
    if (normalize) pn_normalize4(v, red);
    *reinterpret_cast<f32x4*>(patches + p * (PN_PS * PN_PS) + tid * 4) = v;
}

// ---------------------------------------------------------------- conv0 (Cin = 1): VALU, one workgroup per patch
template <int C1>
__global__ __launch_bounds__(256) void pn_conv0_kernel(const float* __restrict__ patches, int normalize, const float* __restrict__ w,
                                                       const float* __restrict__ bias, float* __restrict__ out) {
    __shared__ float red[8];
    __shared__ float t[34][36];
    __shared__ __attribute__((aligned(16))) float ws[9 * C1 + C1];
    const int64_t p = blockIdx.x;
    const int tid = threadIdx.x;
    f32x4 v = *reinterpret_cast<const f32x4*>(patches + p * 1024 + tid * 4);
    if (normalize) pn_normalize4(v, red);
    for (int f = tid; f < 34 * 36; f += 256) (&t[0][0])[f] = 0.f;
    for (int f = tid; f < 10 * C1; f += 256) ws[f] = f < 9 * C1 ? w[f] : bias[f - 9 * C1];
    __syncthreads();
#pragma unroll
    for (int e = 0; e < 4; ++e) t[1 + (tid >> 3)][1 + (tid & 7) * 4 + e] = v[e];
    __syncthreads();
    constexpr int Q = C1 / 4;
    for (int f = tid; f < 1024 * Q; f += 256) {
        const int c4 = (f % Q) * 4, px = f / Q;
        const int y = px >> 5, x = px & 31;
        f32x4 acc = *reinterpret_cast<const f32x4*>(&ws[9 * C1 + c4]);
#pragma unroll
        for (int ky = 0; ky < 3; ++ky)
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) {
                const float a = t[y + ky][x + kx];
                const f32x4 wv = *reinterpret_cast<const f32x4*>(&ws[(ky * 3 + kx) * C1 + c4]);
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[e] = fmaf(wv[e], a, acc[e]);
            }
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[e] = fmaxf(acc[e], 0.f);
        *reinterpret_cast<f32x4*>(out + (p * 1024 + px) * C1 + c4) = acc;
    }
}

// ---------------------------------------------------------------- 3x3 convolution over a batch of small maps
template <int CIN, int COUT, int STRIDE, int SO>
struct PnConv {
    static constexpr int S = SO * STRIDE;                              // input side
    static constexpr int COUTP = COUT < 32 ? 32 : COUT, TN = COUTP / 32;
    static constexpr int NP = SO * SO >= 128 ? 1 : 128 / (SO * SO);    // patches per workgroup
    static constexpr int TR = SO * SO >= 128 ? 128 / SO : SO;          // output rows per patch and workgroup
    static constexpr int BANDS = SO / TR;                              // workgroups per patch (NP == 1)
    static constexpr int IR = (TR - 1) * STRIDE + 3, IC = (SO - 1) * STRIDE + 3;
    static constexpr int KC = (STRIDE == 2 || CIN == 16) ? 16 : 32;    // input channels staged per pass
    static constexpr int LDSC = KC + 4;                                // 16 consecutive pixels hit 16 distinct 4-bank slots (stride 2: 8)
    static constexpr int NSTEPS = 9 * CIN / 8;
};
constexpr int pn_kc(int cin, int stride) { return (stride == 2 || cin == 16) ? 16 : 32; }

// Packed weights per 32-channel output tile jt: [jt][step][lane][4], step = (chunk * 9 + tap) * (KC / 8) + kk, lane l holding
// W[co = 32 jt + (l & 31)][ci = KC chunk + 8 kk + 4 (l >> 5) + e][tap] (zero for co >= Cout).
template <int CIN, int COUT, int STRIDE, int SO>
__global__ __launch_bounds__(256) void pn_conv3x3_kernel(const float* __restrict__ in, const float* __restrict__ wp, const float* __restrict__ bias,
                                                         int n, float* __restrict__ out) {
    using G = PnConv<CIN, COUT, STRIDE, SO>;
    constexpr int TN = G::TN, KC = G::KC, LDSC = G::LDSC, IR = G::IR, IC = G::IC, S = G::S;
    __shared__ __attribute__((aligned(16))) float tile[G::NP * IR * IC * LDSC];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int patch0 = G::NP == 1 ? (int)blockIdx.x / G::BANDS : (int)blockIdx.x * G::NP;
    const int oy0 = G::NP == 1 ? ((int)blockIdx.x % G::BANDS) * G::TR : 0;

    const float* wbase[TN];
#pragma unroll
    for (int j = 0; j < TN; ++j) wbase[j] = wp + ((int64_t)j * G::NSTEPS) * 256 + lane * 4;
    f32x16 acc[TN];
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;

    // the lane's A pixel as an LDS offset at tap (0, 0)
    int a_off;
    {
        const int q = 32 * wave + (lane & 31);
        const int pl = q / (G::TR * SO), rem = q % (G::TR * SO);
        a_off = ((pl * IR + (rem / SO) * STRIDE) * IC + (rem % SO) * STRIDE) * LDSC + 4 * (lane >> 5);
    }

    f32x4 bcur[TN], bnext[TN];
#pragma unroll
    for (int j = 0; j < TN; ++j) bcur[j] = bnext[j] = *reinterpret_cast<const f32x4*>(wbase[j]);
    int s = 0;
    for (int c0 = 0; c0 < CIN; c0 += KC) {
        __syncthreads();
        for (int f = tid; f < G::NP * IR * IC * (KC / 4); f += 256) {
            const int q4 = f % (KC / 4), pix = f / (KC / 4);
            const int c = pix % IC, r = (pix / IC) % IR, pl = pix / (IC * IR);
            const int gy = oy0 * STRIDE - 1 + r, gx = c - 1, patch = patch0 + pl;
            f32x4 v{0.f, 0.f, 0.f, 0.f};
            if (patch < n && gy >= 0 && gy < S && gx >= 0 && gx < S)
                v = *reinterpret_cast<const f32x4*>(in + (((int64_t)patch * S + gy) * S + gx) * CIN + c0 + q4 * 4);
            *reinterpret_cast<f32x4*>(&tile[pix * LDSC + q4 * 4]) = v;
        }
        __syncthreads();
        for (int tap = 0; tap < 9; ++tap) {
            const int toff = ((tap / 3) * IC + (tap % 3)) * LDSC;
#pragma unroll
            for (int kk = 0; kk < KC / 8; ++kk, ++s) {
                if (s + 1 < G::NSTEPS) {
#pragma unroll
                    for (int j = 0; j < TN; ++j) bnext[j] = *reinterpret_cast<const f32x4*>(wbase[j] + (int64_t)(s + 1) * 256);
                }
                const f32x4 a = *reinterpret_cast<const f32x4*>(&tile[a_off + toff + kk * 8]);
#pragma unroll
                for (int e = 0; e < 4; ++e)
#pragma unroll
                    for (int j = 0; j < TN; ++j) acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[e], bcur[j][e], acc[j], 0, 0, 0);
#pragma unroll
                for (int j = 0; j < TN; ++j) bcur[j] = bnext[j];
            }
        }
    }

#pragma unroll
    for (int j = 0; j < TN; ++j) {
        const int co = j * 32 + (lane & 31);
        if (co >= COUT) continue;
        const float bv = bias[co];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int q = 32 * wave + mfma32_row(r, lane);
            const int pl = q / (G::TR * SO), rem = q % (G::TR * SO);
            const int patch = patch0 + pl;
            if (patch >= n) continue;
            out[(((int64_t)patch * SO + oy0 + rem / SO) * SO + rem % SO) * COUT + co] = fmaxf(acc[j][r] + bv, 0.f);
        }
    }
}

// ---------------------------------------------------------------- HardNet tail: [n][8192] x [8192][128] + BN(20)
// grid (ceil(n / 32), 4): 32 patches x 32 channels; wave w sums k in [w K / 4, (w + 1) K / 4); weights [jt][K / 8][lane][4] with
// lane l holding W[co = 32 jt + (l & 31)][k = 8 step + 4 (l >> 5) + e], k = (y * 8 + x) * C + c
constexpr int PN_HK = 64 * 128;
__global__ __launch_bounds__(256) void pn_tail_hardnet_kernel(const float* __restrict__ feat, const float* __restrict__ wp,
                                                              const float* __restrict__ bias, int n, float* __restrict__ out) {
    __shared__ float red[4][32][33];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int p0 = blockIdx.x * 32, jt = blockIdx.y;
    constexpr int STEPS = PN_HK / 8 / 4;               // per wave
    const int row = min(p0 + (lane & 31), n - 1);      // rows past n are computed on a copy of the last one and not stored
    const float* ap = feat + (int64_t)row * PN_HK + (int64_t)wave * STEPS * 8 + 4 * (lane >> 5);
    const float* wt = wp + ((int64_t)jt * (PN_HK / 8) + (int64_t)wave * STEPS) * 256 + lane * 4;
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    f32x4 a = *reinterpret_cast<const f32x4*>(ap), b = *reinterpret_cast<const f32x4*>(wt), an = a, bn = b;
    for (int s = 0; s < STEPS; ++s) {
        if (s + 1 < STEPS) {
            an = *reinterpret_cast<const f32x4*>(ap + (s + 1) * 8);
            bn = *reinterpret_cast<const f32x4*>(wt + (int64_t)(s + 1) * 256);
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[e], b[e], acc, 0, 0, 0);
        a = an;
        b = bn;
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) red[wave][mfma32_row(r, lane)][lane & 31] = acc[r];
    __syncthreads();
    for (int f = tid; f < 1024; f += 256) {
        const int m = f >> 5, c = f & 31;
        if (p0 + m >= n) continue;
        const float v = ((red[0][m][c] + red[1][m][c]) + red[2][m][c]) + red[3][m][c];
        out[(int64_t)(p0 + m) * 128 + jt * 32 + c] = v + bias[jt * 32 + c];
    }
}

// x / max(|x|_2, 1e-12), one wave per descriptor
__global__ __launch_bounds__(256) void pn_l2norm_kernel(int n, float* __restrict__ d) {
    const int lane = threadIdx.x & 63;
    const int64_t p = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (p >= n) return;
    float* r = d + p * 128 + lane * 2;
    const float x = r[0], y = r[1];
    const float nrm = fmaxf(sqrtf(wave_sum(x * x + y * y)), 1e-12f);
    r[0] = x / nrm;
    r[1] = y / nrm;
}

// ---------------------------------------------------------------- AffNet / OriNet tail: one wave per patch, bias, tanh, LAF update
// weights [NOUT][4096] with k = (y * 8 + x) * 64 + c
template <int NOUT>
__global__ __launch_bounds__(256) void pn_tail_laf_kernel(const float* __restrict__ feat, const float* __restrict__ w, const float* __restrict__ bias,
                                                          int n, float* __restrict__ raw, float* __restrict__ lafs) {
    constexpr int K = 64 * 64;
    const int lane = threadIdx.x & 63;
    const int64_t p = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (p >= n) return;
    float acc[NOUT];
#pragma unroll
    for (int o = 0; o < NOUT; ++o) acc[o] = 0.f;
    for (int k = lane * 4; k < K; k += 256) {
        const f32x4 a = *reinterpret_cast<const f32x4*>(feat + p * K + k);
#pragma unroll
        for (int o = 0; o < NOUT; ++o) {
            const f32x4 wv = *reinterpret_cast<const f32x4*>(w + o * K + k);
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[o] = fmaf(a[e], wv[e], acc[o]);
        }
    }
    float y[NOUT];
#pragma unroll
    for (int o = 0; o < NOUT; ++o) y[o] = tanhf(wave_sum(acc[o]) + bias[o]);
    if (lane != 0) return;
    if (raw) {
#pragma unroll
        for (int o = 0; o < NOUT; ++o) raw[p * NOUT + o] = y[o];
    }
    if (!lafs) return;
    float* L = lafs + p * 6;
    const float a00 = L[0], a01 = L[1], a10 = L[3], a11 = L[4];
    if constexpr (NOUT == 3) {
        // A' = [[1 + x0, 0], [x1, 1 + x2]] / sqrt(det); A = scale(A) A' rot(ori(A)), rot(t) = [[cos, sin], [-sin, cos]]
        const float sc = sqrtf(fabsf(a00 * a11 - a01 * a10));
        const float h = hypotf(a00, a01);
        const float c = h > 0.f ? a00 / h : 1.f, s = h > 0.f ? a01 / h : 0.f;          // cos, sin of atan2(a01, a00)
        const float u00 = 1.f + y[0], u10 = y[1], u11 = 1.f + y[2];
        const float k = sc / sqrtf(u00 * u11);
        L[0] = k * (u00 * c);
        L[1] = k * (u00 * s);
        L[3] = k * (u10 * c - u11 * s);
        L[4] = k * (u10 * s + u11 * c);
    } else {
        // A = A rot(atan2(y0 + 1e-8, y1 + 1e-8))
        const float sn = y[0] + 1e-8f, cs = y[1] + 1e-8f;
        const float h = hypotf(sn, cs);
        const float c = h > 0.f ? cs / h : 1.f, s = h > 0.f ? sn / h : 0.f;
        L[0] = a00 * c - a01 * s;
        L[1] = a00 * s + a01 * c;
        L[3] = a10 * c - a11 * s;
        L[4] = a10 * s + a11 * c;
    }
}

// ---------------------------------------------------------------- host side
struct PnNet {
    int c[3];                        // channels at 32 x 32, 16 x 16, 8 x 8
    int nout;                        // outputs of the 8 x 8 convolution
    int cin[5], cout[5], stride[5];  // the five MFMA convolutions (features.3 .. features.15)
    int64_t w0, b0, w[5], b[5], wt, bt, total;
};
bool pn_net(int kind, PnNet& N) {
    if (kind != PN_HARDNET && kind != PN_AFFNET && kind != PN_ORINET) return false;
    const int base = kind == PN_HARDNET ? 32 : 16;
    N.c[0] = base; N.c[1] = 2 * base; N.c[2] = 4 * base;
    N.nout = kind == PN_HARDNET ? 128 : (kind == PN_AFFNET ? 3 : 2);
    const int ci[5] = {N.c[0], N.c[0], N.c[1], N.c[1], N.c[2]}, co[5] = {N.c[0], N.c[1], N.c[1], N.c[2], N.c[2]}, st[5] = {1, 2, 1, 2, 1};
    int64_t o = 0;
    N.w0 = o; o += 9 * base;
    N.b0 = o; o += base;
    for (int l = 0; l < 5; ++l) {
        N.cin[l] = ci[l]; N.cout[l] = co[l]; N.stride[l] = st[l];
        const int coutp = co[l] < 32 ? 32 : co[l];
        N.w[l] = o; o += (int64_t)coutp * 9 * ci[l];
        N.b[l] = o; o += coutp;
    }
    N.wt = o; o += (int64_t)N.nout * 64 * N.c[2];
    N.bt = o; o += og_round_up(N.nout, 4);
    N.total = o;
    return true;
}

template <int CIN, int COUT, int STRIDE, int SO>
void pn_conv(const float* in, const float* P, const PnNet& N, int l, int n, float* out, hipStream_t st) {
    using G = PnConv<CIN, COUT, STRIDE, SO>;
    const unsigned grid = G::NP == 1 ? (unsigned)n * G::BANDS : (unsigned)((n + G::NP - 1) / G::NP);
    hipLaunchKernelGGL((pn_conv3x3_kernel<CIN, COUT, STRIDE, SO>), dim3(grid), dim3(256), 0, st, in, P + N.w[l], P + N.b[l], n, out);
}

template <int C1>
void pn_trunk(const float* patches, int normalize, const float* P, const PnNet& N, int n, float* X, float* Y, hipStream_t st) {
    hipLaunchKernelGGL((pn_conv0_kernel<C1>), dim3(n), dim3(256), 0, st, patches, normalize, P + N.w0, P + N.b0, X);
    pn_conv<C1, C1, 1, 32>(X, P, N, 0, n, Y, st);
    pn_conv<C1, 2 * C1, 2, 16>(Y, P, N, 1, n, X, st);
    pn_conv<2 * C1, 2 * C1, 1, 16>(X, P, N, 2, n, Y, st);
    pn_conv<2 * C1, 4 * C1, 2, 8>(Y, P, N, 3, n, X, st);
    pn_conv<4 * C1, 4 * C1, 1, 8>(X, P, N, 4, n, Y, st);          // features [n][8][8][4 C1] in Y
}

size_t pn_act_bytes(int n) { return (size_t)og_round_up((int64_t)(n < PN_CHUNK ? n : PN_CHUNK) * 1024 * 32 * 4, 256); }

}  // namespace

extern "C" int og_patch_geometry(int32_t H, int32_t W, int32_t* out) {
    if (!out || !pn_image_ok(1, H, W)) return OG_E_INVALID;
    const PnLevels g = pn_levels(H, W);
    out[0] = g.levels;
    out[1] = (int32_t)g.floats;
    for (int l = 0; l < PN_MAX_LEVELS; ++l) {
        out[2 + 2 * l] = l < g.levels ? g.h[l] : 0;
        out[3 + 2 * l] = l < g.levels ? g.w[l] : 0;
    }
    return 0;
}

extern "C" size_t og_patch_workspace_bytes(int32_t batch, int32_t H, int32_t W, int32_t n) {
    size_t img = 0, act = 0;
    if (batch != 0 || H != 0 || W != 0) {
        if (!pn_image_ok(batch, H, W)) return 0;
        img = (size_t)og_round_up((int64_t)batch * H * W * 4, 256);
    }
    if (n < 0) return 0;
    if (n > 0) act = 2 * pn_act_bytes(n);
    const size_t m = img > act ? img : act;
    return m ? m : 256;
}

extern "C" int og_patch_pyramid(int32_t batch, int32_t H, int32_t W, const float* image, float* pyramid, void* workspace_dev, void* stream) {
    og_clear_status();
    if (!image || !pyramid || !workspace_dev || !pn_image_ok(batch, H, W)) return OG_E_INVALID;
    const PnLevels g = pn_levels(H, W);
    if (g.levels == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    float* tmp = (float*)workspace_dev;
    if (hipMemcpyAsync(pyramid, image, (size_t)batch * H * W * 4, hipMemcpyDeviceToDevice, st) != hipSuccess) return og_launch_status();
    for (int l = 0; l + 1 < g.levels; ++l) {
        const float* src = pyramid + (int64_t)batch * g.off[l];
        float* dst = pyramid + (int64_t)batch * g.off[l + 1];
        const int64_t ni = (int64_t)batch * g.h[l] * g.w[l], no = (int64_t)batch * g.h[l + 1] * g.w[l + 1];
        hipLaunchKernelGGL(pn_blur_kernel, dim3((unsigned)((ni + 255) / 256)), dim3(256), 0, st, src, batch, g.h[l], g.w[l], tmp);
        hipLaunchKernelGGL(pn_resize_kernel, dim3((unsigned)((no + 255) / 256)), dim3(256), 0, st, tmp, batch, g.h[l], g.w[l], g.h[l + 1],
                           g.w[l + 1], dst);
    }
    return og_launch_status();
}

extern "C" int og_patch_extract(int32_t batch, int32_t H, int32_t W, int32_t n, const float* pyramid, const float* lafs, int32_t upright,
                                int32_t normalize, float* patches, void* stream) {
    og_clear_status();
    if (!pn_image_ok(batch, H, W) || n < 0 || (int64_t)batch * n > (1ll << 24)) return OG_E_INVALID;
    if (n == 0) return 0;
    if (!pyramid || !lafs || !patches) return OG_E_INVALID;
    if ((uintptr_t)patches % 16) return OG_E_ALIGN;
    const PnLevels g = pn_levels(H, W);
    hipLaunchKernelGGL(pn_extract_kernel, dim3((unsigned)(batch * n)), dim3(256), 0, (hipStream_t)stream, pyramid, g, batch, n, lafs,
                       upright != 0, normalize != 0, patches);
    return og_launch_status();
}

extern "C" size_t og_patchnet_packed_bytes(int32_t kind) {
    PnNet N;
    return pn_net(kind, N) ? (size_t)N.total * 4 : 0;
}

// params (host pointers): for each of the six hidden convolutions features.{0,3,6,9,12,15}: weight [out][in][3][3], then the
// running_mean and running_var of the BatchNorm behind it (18 pointers); then features.19.weight [out][in][8][8] and, HardNet:
// features.20.running_mean, running_var (21 in all); AffNet / OriNet: features.19.bias (20 in all).
extern "C" int og_patchnet_pack(int32_t kind, float bn_eps, const float* const* params, void* packed_host) {
    PnNet N;
    if (!pn_net(kind, N)) return OG_E_SHAPE;
    if (!params || !packed_host) return OG_E_INVALID;
    const int np = kind == PN_HARDNET ? 21 : 20;
    for (int i = 0; i < np; ++i)
        if (!params[i]) return OG_E_INVALID;
    float* P = (float*)packed_host;
    for (int64_t i = 0; i < N.total; ++i) P[i] = 0.f;
    bool finite = true;
    auto put = [&](int64_t o, double v) {
        const float f = (float)v;
        finite = finite && std::isfinite(f);
        P[o] = f;
    };
    // conv -> BN(affine=False): W s, -mean s with s = 1 / sqrt(var + eps)
    auto scale = [&](int conv, int co) { return 1.0 / std::sqrt((double)params[3 * conv + 2][co] + (double)bn_eps); };
    for (int co = 0; co < N.c[0]; ++co) {
        const double sc = scale(0, co);
        for (int t = 0; t < 9; ++t) put(N.w0 + t * N.c[0] + co, (double)params[0][co * 9 + t] * sc);
        put(N.b0 + co, -(double)params[1][co] * sc);
    }
    for (int l = 0; l < 5; ++l) {
        const int Cin = N.cin[l], Cout = N.cout[l], kc = pn_kc(Cin, N.stride[l]);
        const float* w = params[3 * (l + 1)];
        for (int co = 0; co < Cout; ++co) put(N.b[l] + co, -(double)params[3 * (l + 1) + 1][co] * scale(l + 1, co));
        pack_fragments(put, N.w[l], Cout, Cout < 32 ? 32 : Cout, 9 * Cin, [&](int co, int k) {
            int ci, tap;
            conv3x3_k(k, kc, ci, tap);
            return (double)w[((int64_t)co * Cin + ci) * 9 + tap] * scale(l + 1, co);
        });
    }
    const int C = N.c[2], K = 64 * C;
    const float* wt = params[18];
    if (kind == PN_HARDNET) {
        auto tail_scale = [&](int co) { return 1.0 / std::sqrt((double)params[20][co] + (double)bn_eps); };
        for (int co = 0; co < 128; ++co) put(N.bt + co, -(double)params[19][co] * tail_scale(co));
        pack_fragments(put, N.wt, 128, 128, K, [&](int co, int k) { return (double)wt[((int64_t)co * C + k % C) * 64 + k / C] * tail_scale(co); });
    } else {
        for (int co = 0; co < N.nout; ++co) {
            put(N.bt + co, params[19][co]);
            for (int k = 0; k < K; ++k) put(N.wt + (int64_t)co * K + k, wt[((int64_t)co * C + k % C) * 64 + k / C]);
        }
    }
    return finite ? 0 : OG_E_RANGE;
}

// patches [n][32][32] (normalize != 0: raw, the input normalisation runs here).  HardNet: out [n][128].  AffNet / OriNet: out [n][3] /
// [n][2] (the tanh outputs) and / or lafs [n][2][3], updated in place; either may be null, not both.
extern "C" int og_patchnet_forward(int32_t kind, int32_t n, const float* patches, int32_t normalize, const void* packed_dev, float* out,
                                   float* lafs, void* workspace_dev, void* stream) {
    og_clear_status();
    PnNet N;
    if (!pn_net(kind, N)) return OG_E_SHAPE;
    if (n < 0 || n > (1 << 24)) return OG_E_INVALID;
    if (n == 0) return 0;
    if (!patches || !packed_dev || !workspace_dev) return OG_E_INVALID;
    if (kind == PN_HARDNET ? !out : (!out && !lafs)) return OG_E_INVALID;
    if ((uintptr_t)patches % 16 || (uintptr_t)packed_dev % 16 || (uintptr_t)workspace_dev % 16) return OG_E_ALIGN;
    hipStream_t st = (hipStream_t)stream;
    const float* P = (const float*)packed_dev;
    float* X = (float*)workspace_dev;
    float* Y = (float*)((char*)workspace_dev + pn_act_bytes(n));
    for (int c0 = 0; c0 < n; c0 += PN_CHUNK) {
        const int nc = n - c0 < PN_CHUNK ? n - c0 : PN_CHUNK;
        const float* pc = patches + (int64_t)c0 * 1024;
        if (kind == PN_HARDNET) {
            pn_trunk<32>(pc, normalize != 0, P, N, nc, X, Y, st);
            float* oc = out + (int64_t)c0 * 128;
            hipLaunchKernelGGL(pn_tail_hardnet_kernel, dim3((nc + 31) / 32, 4), dim3(256), 0, st, Y, P + N.wt, P + N.bt, nc, oc);
            hipLaunchKernelGGL(pn_l2norm_kernel, dim3((nc + 3) / 4), dim3(256), 0, st, nc, oc);
        } else {
            pn_trunk<16>(pc, normalize != 0, P, N, nc, X, Y, st);
            float* lc = lafs ? lafs + (int64_t)c0 * 6 : nullptr;
            if (kind == PN_AFFNET)
                hipLaunchKernelGGL(pn_tail_laf_kernel<3>, dim3((nc + 3) / 4), dim3(256), 0, st, Y, P + N.wt, P + N.bt, nc,
                                   out ? out + (int64_t)c0 * 3 : nullptr, lc);
            else
                hipLaunchKernelGGL(pn_tail_laf_kernel<2>, dim3((nc + 3) / 4), dim3(256), 0, st, Y, P + N.wt, P + N.bt, nc,
                                   out ? out + (int64_t)c0 * 2 : nullptr, lc);
        }
    }
    return og_launch_status();
}
