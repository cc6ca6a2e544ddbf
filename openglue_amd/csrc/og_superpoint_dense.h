// The dense SuperPoint kernels (conv1a, the 3x3 implicit-GEMM convolution, the cell kernel) and the packed-weight layout, shared by the
// inference path (superpoint.hip) and the training path (superpoint_train.hip).  Internal, not part of the ABI.  Everything lives in
// the unnamed namespace of the including unit.
#pragma once
#include "og_block.h"
#include "og_conv_f32.h"
#include <cmath>

namespace {

constexpr int SP_TH = 8, SP_TW = 16;                 // conv output tile (pre-pool pixels)
constexpr int SP_HALO_H = SP_TH + 2, SP_HALO_W = SP_TW + 2;
constexpr int SP_KC = 32;                            // input channels staged per pass
constexpr int SP_LDSC = SP_KC + 4;                   // padded pixel row in LDS: 16 consecutive pixels hit 16 distinct 4-bank slots
constexpr int SP_CELL_PIX = 32;                      // pixels per cell workgroup
constexpr int SP_CELL_LD = 516;                      // hidden row in LDS (512 + 4)
constexpr int SP_P_TILES = 3, SP_D_TILES = 8;        // convPb: 65 rows padded to 96; convDb: 256
constexpr int SP_D = 256;

struct SpLayout {
    int64_t w1a, b1a;            // conv1a [9][64], [64]
    int64_t w[8], b[8];          // conv1b, 2a, 2b, 3a, 3b, 4a, 4b, heads (Pa | Da): fragment-major, [Cout]
    int64_t wc, bc;              // cell: [11 tiles][32 steps][64][4]; bias [96 | 256]
    int64_t total;
};
constexpr int kCin[8] = {64, 64, 64, 64, 128, 128, 128, 128};
constexpr int kCout[8] = {64, 64, 64, 128, 128, 128, 128, 512};

SpLayout sp_layout() {
    SpLayout L{};
    int64_t o = 0;
    L.w1a = o; o += 9 * 64;
    L.b1a = o; o += 64;
    for (int i = 0; i < 8; ++i) {
        L.w[i] = o; o += (int64_t)kCout[i] * 9 * kCin[i];
        L.b[i] = o; o += kCout[i];
    }
    L.wc = o; o += (int64_t)(SP_P_TILES + SP_D_TILES) * 32 * 256;
    L.bc = o; o += 32 * SP_P_TILES + SP_D;
    L.total = o;
    return L;
}

// ---------------------------------------------------------------- conv1a (Cin = 1): VALU
__global__ __launch_bounds__(256) void sp_conv1a_kernel(const float* __restrict__ img, const float* __restrict__ w,
                                                        const float* __restrict__ bias, int B, int H, int W, float* __restrict__ out) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t total = (int64_t)B * H * W * 16;
    if (t >= total) return;
    const int c4 = (int)(t & 15) * 4;
    const int64_t p = t >> 4;
    const int x = (int)(p % W), y = (int)((p / W) % H);
    const int64_t b = p / ((int64_t)W * H);
    const float* im = img + b * H * W;
    f32x4 acc = *reinterpret_cast<const f32x4*>(bias + c4);
#pragma unroll
    for (int ky = 0; ky < 3; ++ky)
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
            const int yy = y + ky - 1, xx = x + kx - 1;
            const float v = (yy >= 0 && yy < H && xx >= 0 && xx < W) ? im[(int64_t)yy * W + xx] : 0.f;
            const f32x4 wv = *reinterpret_cast<const f32x4*>(w + (ky * 3 + kx) * 64 + c4);
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[e] = fmaf(wv[e], v, acc[e]);
        }
#pragma unroll
    for (int e = 0; e < 4; ++e) acc[e] = fmaxf(acc[e], 0.f);
    *reinterpret_cast<f32x4*>(out + p * 64 + c4) = acc;
}

// ---------------------------------------------------------------- 3x3 convolution, implicit GEMM on fp32 MFMA
// M = 128 output pixels (8 rows x 16 columns), N = BN channels, K = 9 taps x Cin.  4 waves as 2 x 2: wave (wm, wn) owns tile rows
// 4 wm .. 4 wm + 3 (two 32-pixel MFMA tiles of two image rows each) and channels wn * BN/2 ..  A 32x32x2 MFMA tile row m is pixel
// (row m >> 4, column m & 15) of its two-row band, so lane l's accumulator registers r, r+1, r+8, r+9 (r in {0, 2, 4, 6}) are the
// four pixels of one 2x2 pooling window (mfma32_row): the pool is a register max.
// Packed weights, per 32-channel output tile jt: [jt][step][lane][4] with step = (chunk * 9 + tap) * 4 + kk and
// lane l holding W[co = 32 jt + (l & 31)][ci = 32 chunk + 8 kk + 4 (l >> 5) + e][tap] -- one coalesced 1 KiB read per fragment.
template <int BN, bool POOL>
__global__ __launch_bounds__(256, 2) void sp_conv3x3_kernel(const float* __restrict__ in, const float* __restrict__ wp,
                                                            const float* __restrict__ bias, int B, int H, int W, int Cin, int Cout,
                                                            float* __restrict__ out) {
    constexpr int TM = 2, TN = BN / 64;
    __shared__ __attribute__((aligned(16))) float tile[SP_HALO_H * SP_HALO_W * SP_LDSC];
    const int tiles_x = (W + SP_TW - 1) / SP_TW, tiles_y = (H + SP_TH - 1) / SP_TH;
    int id = blockIdx.x;
    const int tx0 = (id % tiles_x) * SP_TW;
    id /= tiles_x;
    const int ty0 = (id % tiles_y) * SP_TH;
    const int b = id / tiles_y;
    const int n0 = blockIdx.y * BN;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int nsteps = 9 * Cin / 8;
    const float* inb = in + (int64_t)b * H * W * Cin;

    const float* wbase[TN];
#pragma unroll
    for (int j = 0; j < TN; ++j) wbase[j] = wp + ((int64_t)((n0 + wn * (BN / 2)) / 32 + j) * nsteps) * 256 + lane * 4;

    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    // the lane's A pixel in each of its M tiles, as an LDS offset at tap (0, 0) of the halo tile
    int a_off[TM];
#pragma unroll
    for (int i = 0; i < TM; ++i) {
        const int m = lane & 31;
        const int ry = 4 * wm + 2 * i + (m >> 4), rx = m & 15;
        a_off[i] = (ry * SP_HALO_W + rx) * SP_LDSC + 4 * (lane >> 5);
    }

    f32x4 bcur[TN], bnext[TN];
#pragma unroll
    for (int j = 0; j < TN; ++j) bcur[j] = *reinterpret_cast<const f32x4*>(wbase[j]);
    int s = 0;
    for (int c0 = 0; c0 < Cin; c0 += SP_KC) {
        __syncthreads();
        for (int f = tid; f < SP_HALO_H * SP_HALO_W * (SP_KC / 4); f += 256) {
            const int q = f & 7, p = f >> 3;
            const int py = p / SP_HALO_W, px = p - py * SP_HALO_W;
            const int gy = ty0 - 1 + py, gx = tx0 - 1 + px;
            f32x4 v{0.f, 0.f, 0.f, 0.f};
            if (gy >= 0 && gy < H && gx >= 0 && gx < W) v = *reinterpret_cast<const f32x4*>(inb + ((int64_t)gy * W + gx) * Cin + c0 + q * 4);
            *reinterpret_cast<f32x4*>(&tile[p * SP_LDSC + q * 4]) = v;
        }
        __syncthreads();
        for (int tap = 0; tap < 9; ++tap) {
            const int toff = ((tap / 3) * SP_HALO_W + (tap % 3)) * SP_LDSC;
#pragma unroll
            for (int kk = 0; kk < 4; ++kk, ++s) {
                if (s + 1 < nsteps) {
#pragma unroll
                    for (int j = 0; j < TN; ++j) bnext[j] = *reinterpret_cast<const f32x4*>(wbase[j] + (int64_t)(s + 1) * 256);
                }
                f32x4 a[TM];
#pragma unroll
                for (int i = 0; i < TM; ++i) a[i] = *reinterpret_cast<const f32x4*>(&tile[a_off[i] + toff + kk * 8]);
#pragma unroll
                for (int e = 0; e < 4; ++e)
#pragma unroll
                    for (int i = 0; i < TM; ++i)
#pragma unroll
                        for (int j = 0; j < TN; ++j)
                            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i][e], bcur[j][e], acc[i][j], 0, 0, 0);
#pragma unroll
                for (int j = 0; j < TN; ++j) bcur[j] = bnext[j];
            }
        }
    }

#pragma unroll
    for (int j = 0; j < TN; ++j) {
        const int co = n0 + wn * (BN / 2) + j * 32 + (lane & 31);
        const float bv = bias[co];
#pragma unroll
        for (int i = 0; i < TM; ++i) {
            const int band = ty0 + 4 * wm + 2 * i;              // first image row of this MFMA tile
            if constexpr (POOL) {
                const int Hp = H / 2, Wp = W / 2;
                const int py = band / 2;
                if (py >= Hp) continue;
#pragma unroll
                for (int r = 0; r < 8; r += 2) {
                    const int m = mfma32_row(r, lane);           // even column, upper row of the window
                    const int px = (tx0 + (m & 15)) / 2;
                    if (px >= Wp) continue;
                    float v = fmaxf(fmaxf(acc[i][j][r], acc[i][j][r + 1]), fmaxf(acc[i][j][r + 8], acc[i][j][r + 9]));
                    v = fmaxf(v + bv, 0.f);
                    out[(((int64_t)b * Hp + py) * Wp + px) * Cout + co] = v;
                }
            } else {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int m = mfma32_row(r, lane);
                    const int y = band + (m >> 4), x = tx0 + (m & 15);
                    if (y >= H || x >= W) continue;
                    out[(((int64_t)b * H + y) * W + x) * Cout + co] = fmaxf(acc[i][j][r] + bv, 0.f);
                }
            }
        }
    }
}

// ---------------------------------------------------------------- cell: convPb + softmax + depth-to-space, convDb + L2 norm
// 32 pixels per workgroup; their 512 hidden channels sit in LDS.  11 output tiles of 32 (3 for the 65 logits, zero-padded to 96;
// 8 for the 256 descriptor channels), wave w takes tiles w, w + 4, w + 8.  The tiles' results go back to LDS, then one thread per
// pixel reduces (max / sum of exp over 65, sum of squares over 256) and all threads write the outputs coalesced.
__global__ __launch_bounds__(256, 1) void sp_cell_kernel(const float* __restrict__ hidden, const float* __restrict__ wc,
                                                         const float* __restrict__ bc, int npix, int Hc, int Wc,
                                                         float* __restrict__ heat, float* __restrict__ desc) {
    constexpr int LD_P = 97, LD_D = SP_D + 4;
    __shared__ __attribute__((aligned(16))) float lds[SP_CELL_PIX * SP_CELL_LD];
    __shared__ float stat[SP_CELL_PIX][2];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t p0 = (int64_t)blockIdx.x * SP_CELL_PIX;
    for (int f = tid; f < SP_CELL_PIX * 128; f += 256) {
        const int r = f >> 7, q = f & 127;
        f32x4 v{0.f, 0.f, 0.f, 0.f};
        if (p0 + r < npix) v = *reinterpret_cast<const f32x4*>(hidden + (p0 + r) * 512 + q * 4);
        *reinterpret_cast<f32x4*>(&lds[r * SP_CELL_LD + q * 4]) = v;
    }
    __syncthreads();
    f32x16 acc[3];
    int tiles[3], nt = 0;
    for (int t = wave; t < SP_P_TILES + SP_D_TILES; t += 4) tiles[nt++] = t;
#pragma unroll
    for (int u = 0; u < 3; ++u)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[u][r] = 0.f;
    const int a_row = (lane & 31) * SP_CELL_LD + 4 * (lane >> 5);
#pragma unroll
    for (int u = 0; u < 3; ++u) {
        if (u >= nt) break;
        const int t = tiles[u];
        const int kbase = t < SP_P_TILES ? 0 : 256;
        const float* wt = wc + (int64_t)t * 32 * 256 + lane * 4;
        f32x4 bcur = *reinterpret_cast<const f32x4*>(wt), bnext;
        for (int s = 0; s < 32; ++s) {
            if (s + 1 < 32) bnext = *reinterpret_cast<const f32x4*>(wt + (s + 1) * 256);
            const f32x4 a = *reinterpret_cast<const f32x4*>(&lds[a_row + kbase + s * 8]);
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[u] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[e], bcur[e], acc[u], 0, 0, 0);
            bcur = bnext;
        }
    }
    __syncthreads();                       // hidden no longer needed: the logits and descriptors reuse the LDS
    float* lp = lds;                       // [32][LD_P]
    float* ld = lds + SP_CELL_PIX * LD_P;  // [32][LD_D]
#pragma unroll
    for (int u = 0; u < 3; ++u) {
        if (u >= nt) break;
        const int t = tiles[u];
        const int col = (t < SP_P_TILES ? t : t - SP_P_TILES) * 32 + (lane & 31);
        const float bv = bc[(t < SP_P_TILES ? 0 : 32 * SP_P_TILES) + col];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = mfma32_row(r, lane);
            if (t < SP_P_TILES) {
                if (col < 65) lp[row * LD_P + col] = acc[u][r] + bv;
            } else {
                ld[row * LD_D + col] = acc[u][r] + bv;
            }
        }
    }
    __syncthreads();
    if (tid < SP_CELL_PIX) {
        const float* l = lp + tid * LD_P;
        float mx = l[0];
        for (int c = 1; c < 65; ++c) mx = fmaxf(mx, l[c]);
        float sum = 0.f;
        for (int c = 0; c < 65; ++c) sum += expf(l[c] - mx);
        stat[tid][0] = mx;
        stat[tid][1] = sum;
    } else if (tid >= 64 && tid < 64 + SP_CELL_PIX) {
        const float* d = ld + (tid - 64) * LD_D;
        float ss = 0.f;
        for (int c = 0; c < SP_D; ++c) ss = fmaf(d[c], d[c], ss);
        lp[(tid - 64) * LD_P + 96] = sqrtf(ss);             // slot 96 of the logit row is free (65 used)
    }
    __syncthreads();
    const int Hh = Hc * 8, Wh = Wc * 8;
    for (int f = tid; f < SP_CELL_PIX * 64; f += 256) {
        const int r = f >> 6, c = f & 63;
        const int64_t p = p0 + r;
        if (p >= npix) continue;
        const int64_t b = p / ((int64_t)Hc * Wc);
        const int rem = (int)(p - b * Hc * Wc), cy = rem / Wc, cx = rem - cy * Wc;
        heat[(b * Hh + cy * 8 + (c >> 3)) * Wh + cx * 8 + (c & 7)] = expf(lp[r * LD_P + c] - stat[r][0]) / stat[r][1];
    }
    for (int f = tid; f < SP_CELL_PIX * (SP_D / 4); f += 256) {
        const int r = f / (SP_D / 4), c4 = (f % (SP_D / 4)) * 4;
        const int64_t p = p0 + r;
        if (p >= npix) continue;
        const float nrm = lp[r * LD_P + 96];
        f32x4 v;
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = ld[r * LD_D + c4 + e] / nrm;
        *reinterpret_cast<f32x4*>(desc + p * SP_D + c4) = v;
    }
}

// ---------------------------------------------------------------- host side
struct Dims {
    int H2, W2, H4, W4, Hc, Wc;
};
Dims dims(int H, int W) { return {H / 2, W / 2, H / 4, W / 4, H / 8, W / 8}; }

bool dense_shape_ok(int B, int H, int W) { return B > 0 && H >= 8 && W >= 8 && (int64_t)B * H * W <= (1ll << 26); }

template <int BN, bool POOL>
void conv(const float* in, const float* w, const float* bias, int B, int H, int W, int Cin, int Cout, float* out, hipStream_t st) {
    const int tiles = ((W + SP_TW - 1) / SP_TW) * ((H + SP_TH - 1) / SP_TH) * B;
    hipLaunchKernelGGL((sp_conv3x3_kernel<BN, POOL>), dim3(tiles, Cout / BN), dim3(256), 0, st, in, w, bias, B, H, W, Cin, Cout, out);
}

}  // namespace
