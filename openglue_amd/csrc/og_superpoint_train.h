// What the two SuperPoint training units share: the 3x3 K loop for any source of input pixels, the layer table, the split of a
// weight-gradient launch and the split-order reduction.  Used by superpoint_train.hip (SuperPointNet) and superpoint_bn_train.hip
// (SuperPointNetBn).  Internal, not part of the ABI.  Everything lives in the unnamed namespace of the including unit.
#pragma once
#include "og_superpoint_dense.h"
#include <algorithm>

namespace {

constexpr int SPW_LD = 36;                           // wgrad LDS row: 32 channels + 4, f32x4 stores stay aligned
constexpr int SP_LAYERS = 8;
constexpr bool kPooled[SP_LAYERS] = {true, false, true, false, true, false, false, false};

// ---------------------------------------------------------------- the K loop of the 3x3 convolution for any source of input pixels
// load(gy, gx, c) returns channels c .. c + 3 of pixel (gy, gx) of the workgroup's image (called for pixels inside the image only; the
// halo outside is zero).  Same tiling, packed-weight order and, unless CHUNKED, MFMA sequence as sp_conv3x3_kernel, hence the same bits.  (Routing the
// inference kernel itself through this function costs it an occupancy step -- 116 -> 162 VGPRs at BN = 128 -- so it keeps its body.)
struct SpTile {
    int b, ty0, tx0, n0;         // image, first row / column of the 8 x 16 tile, first output channel
    int lane, wm, wn;
};
__device__ __forceinline__ SpTile sp_tile(int H, int W, int BN) {
    const int tiles_x = (W + SP_TW - 1) / SP_TW, tiles_y = (H + SP_TH - 1) / SP_TH;
    SpTile t;
    int id = blockIdx.x;
    t.tx0 = (id % tiles_x) * SP_TW;
    id /= tiles_x;
    t.ty0 = (id % tiles_y) * SP_TH;
    t.b = id / tiles_y;
    t.n0 = blockIdx.y * BN;
    const int wave = threadIdx.x >> 6;
    t.lane = threadIdx.x & 63;
    t.wm = wave >> 1;
    t.wn = wave & 1;
    return t;
}

// CHUNKED (the data gradient): every pass of SP_KC input channels x 9 taps (288 products) is summed in an accumulator of its own and
// then added to the total, instead of one chain over all 9 * Cin products.  With K = 9 x 512 at the heads a single fp32 chain is
// 7 - 8x as far from float64 as ATen's blocked sums (tests/test_gpu_superpoint_train_forms.py); chunked it is a sum of 16 short chains.
template <int BN, bool CHUNKED = false, class Load>
__device__ __forceinline__ void sp_conv3x3_accumulate(Load load, const float* __restrict__ wp, int H, int W, int Cin, const SpTile& t,
                                                      float* tile, f32x16 (&acc)[2][BN / 64]) {
    constexpr int TM = 2, TN = BN / 64;
    const int tid = threadIdx.x, lane = t.lane, wm = t.wm, wn = t.wn, ty0 = t.ty0, tx0 = t.tx0;
    const int nsteps = 9 * Cin / 8;

    const float* wbase[TN];
#pragma unroll
    for (int j = 0; j < TN; ++j) wbase[j] = wp + ((int64_t)((t.n0 + wn * (BN / 2)) / 32 + j) * nsteps) * 256 + lane * 4;

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
            if (gy >= 0 && gy < H && gx >= 0 && gx < W) v = load(gy, gx, c0 + q * 4);
            *reinterpret_cast<f32x4*>(&tile[p * SP_LDSC + q * 4]) = v;
        }
        __syncthreads();
        f32x16 part[TM][TN];                         // CHUNKED: this pass alone
        if constexpr (CHUNKED) {
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j)
#pragma unroll
                    for (int r = 0; r < 16; ++r) part[i][j][r] = 0.f;
        }
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
                        for (int j = 0; j < TN; ++j) {
                            if constexpr (CHUNKED) part[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i][e], bcur[j][e], part[i][j], 0, 0, 0);
                            else acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i][e], bcur[j][e], acc[i][j], 0, 0, 0);
                        }
#pragma unroll
                for (int j = 0; j < TN; ++j) bcur[j] = bnext[j];
            }
        }
        if constexpr (CHUNKED) {
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j)
#pragma unroll
                    for (int r = 0; r < 16; ++r) acc[i][j][r] += part[i][j][r];
        }
    }
}

// out[i] = part[0][i] + part[1][i] + ... in split order
__global__ __launch_bounds__(256) void sp_reduce_parts_kernel(const float* __restrict__ part, int S, int64_t n, float* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float v = 0.f;
#pragma unroll 8
    for (int s = 0; s < S; ++s) v += part[(int64_t)s * n + i];          // loads in flight together, added in split order
    out[i] = v;
}

void layer_dims(int j, int H, int W, int& h, int& w) {       // resolution at which layer j convolves
    const int sh = j < 1 ? 0 : j < 3 ? 1 : j < 5 ? 2 : 3;
    h = H >> sh;
    w = W >> sh;
}

// split of a weight-gradient launch over the pixel tiles of a layer
struct Split {
    int tiles_per, S;
};
Split sp_wgrad_split(int B, int h, int w, int Cin, int Cout, int target_wgs) {
    const int total = B * ((h + SP_TH - 1) / SP_TH) * ((w + SP_TW - 1) / SP_TW);
    const int blocks = (Cin / 32) * (Cout / 32);
    int S = (target_wgs + blocks - 1) / blocks;
    S = S < 1 ? 1 : S > total ? total : S;
    const int per = (total + S - 1) / S;
    return {per, (total + per - 1) / per};
}

int64_t dgrad_offset(int j) {
    int64_t o = 0;
    for (int i = 0; i < j; ++i) o += (int64_t)kCout[i] * 9 * kCin[i];
    return o;
}

void reduce_parts(const float* part, int S, int64_t n, float* out, hipStream_t st) {
    hipLaunchKernelGGL(sp_reduce_parts_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, part, S, n, out);
}

}  // namespace
