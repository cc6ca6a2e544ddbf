// What the two SuperPoint training units share -- superpoint_train.hip (SuperPointNet, policy SpPlain) and superpoint_bn_train.hip
// (SuperPointNetBn, policy SpBn): the 3x3 K loop for any source of input pixels, the one body of
// every backward kernel (weight gradient, data gradient, conv1a weight gradient, dump, split-order reduction), the layer table, the
// launch constants, the workspace layout of a backward and the one host loop over the layers.  Internal, not part of the ABI.
// Everything lives in the unnamed namespace of the including unit.
//
// A unit describes its network by a policy type `Net`; the kernels are templates over it, so an instance names its network:
//   Net::Grad, Net::In                                  kernel arguments: what the gradient of a layer's pre-activation output, and the
//                                                       layer's input activation, are formed from
//   Net::grad_at<POOLED>(gs, b, H, W, C, y, x, c)       channels c .. c + 3 of that gradient at pixel (y, x) of the layer's H x W map
//   Net::input_at<INPOOL>(xs, b, H, W, C, y, x, c)      channels c .. c + 3 of the input activation at that pixel
//   Net::grad1a(gs, co)                                 conv1a: a callable p -> that gradient at flat pixel p, channel co
//   Net::dx_value(xs, o, v)                             what the data gradient stores at element o of the input for the sum v
//   Net::kBias                                          the convolution biases get a gradient (summed from the A operands)
//   Net::kPoolOnLoad                                    input_at<true> exists: a layer behind a pool forms the pooled input on load
//   Net::kDump1a                                        layer_grads opens with the plane of conv1a's gradient
// and the host loop by an object with grad(L, g, h, w) -> Net::Grad (L = 0 conv1a, j + 1 the MFMA layer j; it may launch what has
// to precede the layer's kernels) and input(j) -> Net::In.
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

// debug: the full-resolution pre-activation gradient of a layer as every kernel below sees it, out [B][H][W][C]
template <class Net, bool POOLED>
__global__ __launch_bounds__(256) void sp_grad_dump_kernel(typename Net::Grad gs, int B, int H, int W, int C, float* __restrict__ out) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int c4 = C / 4;
    if (t >= (int64_t)B * H * W * c4) return;
    const int c = (int)(t % c4) * 4;
    const int64_t p = t / c4;
    const int x = (int)(p % W), y = (int)((p / W) % H), b = (int)(p / ((int64_t)W * H));
    *reinterpret_cast<f32x4*>(out + p * C + c) = Net::template grad_at<POOLED>(gs, b, H, W, C, y, x, c);
}

// ---------------------------------------------------------------- data gradient of a 3x3 layer
// dx [B][H][W][Cx] = conv3x3(G, W^T flipped), stored through Net::dx_value (xs: the layer's input, same shape as dx).  Cg = the layer's
// output channels (the K axis here), wp = the layer's block of the dgrad blob (og_superpoint_train_pack).
template <class Net, int BN, bool POOLED>
__global__ __launch_bounds__(256, 2) void sp_dgrad_kernel(typename Net::Grad gs, typename Net::In xs, const float* __restrict__ wp, int B,
                                                          int H, int W, int Cg, int Cx, float* __restrict__ dx) {
    constexpr int TM = 2, TN = BN / 64;
    __shared__ __attribute__((aligned(16))) float tile[SP_HALO_H * SP_HALO_W * SP_LDSC];
    const SpTile t = sp_tile(H, W, BN);
    const int b = t.b, lane = t.lane;
    f32x16 acc[TM][TN];
    sp_conv3x3_accumulate<BN, true>([=](int gy, int gx, int c) { return Net::template grad_at<POOLED>(gs, b, H, W, Cg, gy, gx, c); }, wp, H, W,
                                    Cg, t, tile, acc);
#pragma unroll
    for (int j = 0; j < TN; ++j) {
        const int co = t.n0 + t.wn * (BN / 2) + j * 32 + (lane & 31);
#pragma unroll
        for (int i = 0; i < TM; ++i) {
            const int band = t.ty0 + 4 * t.wm + 2 * i;              // first image row of this MFMA tile
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int m = mfma32_row(r, lane);
                const int y = band + (m >> 4), x = t.tx0 + (m & 15);
                if (y >= H || x >= W) continue;
                const int64_t o = (((int64_t)b * H + y) * W + x) * Cx + co;
                dx[o] = Net::dx_value(xs, o, acc[i][j][r]);
            }
        }
    }
}

// ---------------------------------------------------------------- weight and bias gradient of a 3x3 layer, split over pixel tiles
// Workgroup (split s, block (co0, ci0)): tiles [s * tiles_per, (s + 1) * tiles_per) of the B * tiles_y * tiles_x pixel tiles.
// MFMA: D[co][ci] += A[co][k] B[k][ci] with k a pixel pair: lane l gives A = G[pixel 2 kk + (l >> 5)][co0 + (l & 31)] and, per tap,
// B = x[that pixel + tap][ci0 + (l & 31)].  part_w [S][Cout][Cin][9]; Net::kBias: part_b [S][Cout] (written by the ci0 == 0 workgroups).
template <class Net, bool POOLED, bool INPOOL>
__global__ __launch_bounds__(256) void sp_wgrad_kernel(typename Net::Grad gs, typename Net::In xs, int B, int H, int W, int Cin, int Cout,
                                                       int tiles_per, float* __restrict__ part_w, float* __restrict__ part_b) {
    __shared__ __attribute__((aligned(16))) float gl[SP_TH * SP_TW * SPW_LD];
    __shared__ __attribute__((aligned(16))) float xl[SP_HALO_H * SP_HALO_W * SPW_LD];      // also the 4 x 1024 floats of the wave reduction
    static_assert(SP_HALO_H * SP_HALO_W * SPW_LD >= 4 * 1024, "the wave reduction reuses the halo tile");
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int s = blockIdx.x, ci_tiles = Cin / 32;
    const int co0 = ((int)blockIdx.y / ci_tiles) * 32, ci0 = ((int)blockIdx.y % ci_tiles) * 32;
    const int tiles_x = (W + SP_TW - 1) / SP_TW, tiles_y = (H + SP_TH - 1) / SP_TH;
    const int total = B * tiles_y * tiles_x;
    const int t_begin = s * tiles_per, t_end = min(total, t_begin + tiles_per);

    f32x16 acc[9];
#pragma unroll
    for (int tap = 0; tap < 9; ++tap)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[tap][r] = 0.f;
    float bsum = 0.f;

    for (int t = t_begin; t < t_end; ++t) {
        int id = t;
        const int tx0 = (id % tiles_x) * SP_TW;
        id /= tiles_x;
        const int ty0 = (id % tiles_y) * SP_TH;
        const int b = id / tiles_y;
        __syncthreads();
        for (int f = tid; f < SP_TH * SP_TW * 8; f += 256) {
            const int q = f & 7, p = f >> 3;
            const int y = ty0 + (p >> 4), xx = tx0 + (p & 15);
            f32x4 v{0.f, 0.f, 0.f, 0.f};
            if (y < H && xx < W) v = Net::template grad_at<POOLED>(gs, b, H, W, Cout, y, xx, co0 + q * 4);
            *reinterpret_cast<f32x4*>(&gl[p * SPW_LD + q * 4]) = v;
        }
        for (int f = tid; f < SP_HALO_H * SP_HALO_W * 8; f += 256) {
            const int q = f & 7, p = f >> 3;
            const int py = p / SP_HALO_W, px = p - py * SP_HALO_W;
            const int gy = ty0 - 1 + py, gx = tx0 - 1 + px;
            f32x4 v{0.f, 0.f, 0.f, 0.f};
            if (gy >= 0 && gy < H && gx >= 0 && gx < W) v = Net::template input_at<INPOOL>(xs, b, H, W, Cin, gy, gx, ci0 + q * 4);
            *reinterpret_cast<f32x4*>(&xl[p * SPW_LD + q * 4]) = v;
        }
        __syncthreads();
#pragma unroll 4
        for (int kk = 0; kk < 16; ++kk) {
            const int prow = 2 * wave + (kk >> 3), pcol = 2 * (kk & 7) + (lane >> 5);
            const float av = gl[(prow * SP_TW + pcol) * SPW_LD + (lane & 31)];
            if constexpr (Net::kBias) bsum += av;
            const float* xb = &xl[(prow * SP_HALO_W + pcol) * SPW_LD + (lane & 31)];
#pragma unroll
            for (int tap = 0; tap < 9; ++tap)
                acc[tap] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, xb[((tap / 3) * SP_HALO_W + (tap % 3)) * SPW_LD], acc[tap], 0, 0, 0);
        }
    }

    // the four waves in wave order, one tap at a time through LDS
    float* red = xl;
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
        __syncthreads();
#pragma unroll
        for (int r = 0; r < 16; ++r) red[wave * 1024 + r * 64 + lane] = acc[tap][r];
        __syncthreads();
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int e = tid + 256 * u;
            const float v = ((red[e] + red[1024 + e]) + red[2048 + e]) + red[3072 + e];
            const int co = co0 + mfma32_row(e >> 6, e & 63), ci = ci0 + (e & 31);
            part_w[(((int64_t)s * Cout + co) * Cin + ci) * 9 + tap] = v;
        }
    }
    if constexpr (Net::kBias) {
        __shared__ float bl[4][32];
        bsum += __shfl_xor(bsum, 32, 64);
        if (lane < 32) bl[wave][lane] = bsum;
        __syncthreads();
        if (ci0 == 0 && tid < 32) part_b[(int64_t)s * Cout + co0 + tid] = ((bl[0][tid] + bl[1][tid]) + bl[2][tid]) + bl[3][tid];
    }
}

// conv1a: dW[co][tap] = sum over pixels of G[p][co] img[p + tap] and, with Net::kBias, db[co] = sum of G[p][co].  Workgroup s owns pixels
// [s * pix_per, (s + 1) * pix_per) of B * H * W; thread (co = tid & 63, sub = tid >> 6) walks every fourth pixel of the range.
template <class Net>
__global__ __launch_bounds__(256) void sp_wgrad1a_kernel(typename Net::Grad gs, const float* __restrict__ img, int B, int H, int W,
                                                         int64_t pix_per, float* __restrict__ part_w, float* __restrict__ part_b) {
    constexpr int NA = Net::kBias ? 10 : 9;          // the nine taps, then the bias
    __shared__ float red[4][64][NA];
    const int tid = threadIdx.x, co = tid & 63, sub = tid >> 6;
    const int64_t total = (int64_t)B * H * W;
    const int64_t p0 = (int64_t)blockIdx.x * pix_per, p1 = min(total, p0 + pix_per);
    const auto g_at = Net::grad1a(gs, co);
    float acc[NA];
#pragma unroll
    for (int i = 0; i < NA; ++i) acc[i] = 0.f;
    for (int64_t p = p0 + sub; p < p1; p += 4) {
        const int x = (int)(p % W), y = (int)((p / W) % H);
        const float* im = img + (p / ((int64_t)W * H)) * H * W;
        const float gv = g_at(p);
        if constexpr (Net::kBias) acc[9] += gv;
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            const int yy = y + tap / 3 - 1, xx = x + tap % 3 - 1;
            const float v = (yy >= 0 && yy < H && xx >= 0 && xx < W) ? im[(int64_t)yy * W + xx] : 0.f;
            acc[tap] = __builtin_fmaf(gv, v, acc[tap]);
        }
    }
#pragma unroll
    for (int i = 0; i < NA; ++i) red[sub][co][i] = acc[i];
    __syncthreads();
    if (tid < 64) {
#pragma unroll
        for (int i = 0; i < NA; ++i) {
            const float v = ((red[0][tid][i] + red[1][tid][i]) + red[2][tid][i]) + red[3][tid][i];
            if (i < 9) part_w[((int64_t)blockIdx.x * 64 + tid) * 9 + i] = v;
            else part_b[(int64_t)blockIdx.x * 64 + tid] = v;
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

// ---------------------------------------------------------------- host side
constexpr int SPW_TARGET_WGS = 512;                  // workgroups a weight-gradient launch aims at (two per CU)
constexpr int64_t SP_1A_PIX = 1024;                  // pixels per conv1a weight-gradient workgroup

void layer_dims(int j, int H, int W, int& h, int& w) {       // resolution at which layer j convolves
    const int sh = j < 1 ? 0 : j < 3 ? 1 : j < 5 ? 2 : 3;
    h = H >> sh;
    w = W >> sh;
}

int conv_tiles(int B, int h, int w) { return B * ((h + SP_TH - 1) / SP_TH) * ((w + SP_TW - 1) / SP_TW); }        // 8 x 16 pixel tiles of a layer
int wgrad1a_splits(int B, int H, int W) { return (int)(((int64_t)B * H * W + SP_1A_PIX - 1) / SP_1A_PIX); }

// split of a weight-gradient launch over the pixel tiles of a layer
struct Split {
    int tiles_per, S;
};
Split wgrad_split(int B, int h, int w, int Cin, int Cout) {
    const int total = conv_tiles(B, h, w);
    const int blocks = (Cin / 32) * (Cout / 32);
    int S = (SPW_TARGET_WGS + blocks - 1) / blocks;
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

// The part of a backward's workspace (floats, from offset o) that both networks lay out alike: the two data-gradient buffers that the
// layers write in turn and the weight-gradient partials of the largest launch, with the bias partials behind them where `bias`.
struct BackwardWs {
    int64_t buf_even, buf_odd, part, total;
};
BackwardWs backward_layout(int64_t o, int B, int H, int W, bool bias) {
    const Dims d = dims(H, W);
    BackwardWs w{};
    w.buf_even = o; o += og_round_up((int64_t)B * H * W * 64, 64);
    w.buf_odd = o; o += og_round_up(std::max((int64_t)B * d.H2 * d.W2 * 64, (int64_t)B * d.Hc * d.Wc * 128), 64);
    int64_t part = (int64_t)wgrad1a_splits(B, H, W) * 64 * (bias ? 10 : 9);
    for (int j = 0; j < SP_LAYERS; ++j) {
        int h, ww;
        layer_dims(j, H, W, h, ww);
        part = std::max(part, (int64_t)wgrad_split(B, h, ww, kCin[j], kCout[j]).S * ((int64_t)kCout[j] * kCin[j] * 9 + (bias ? kCout[j] : 0)));
    }
    w.part = o; o += og_round_up(part, 64);
    w.total = o;
    return w;
}

template <class Net>
void grad_dump(const typename Net::Grad& gs, bool pooled, int B, int h, int w, int C, float* out, hipStream_t st) {
    const dim3 grid((unsigned)(((int64_t)B * h * w * (C / 4) + 255) / 256));
    if (pooled) hipLaunchKernelGGL((sp_grad_dump_kernel<Net, true>), grid, dim3(256), 0, st, gs, B, h, w, C, out);
    else hipLaunchKernelGGL((sp_grad_dump_kernel<Net, false>), grid, dim3(256), 0, st, gs, B, h, w, C, out);
}

template <class Net, int BN>
void dgrad(const typename Net::Grad& gs, const typename Net::In& xs, bool pooled, const float* wp, int B, int h, int w, int Cg, int Cx, float* dx,
           hipStream_t st) {
    const dim3 grid(conv_tiles(B, h, w), Cx / BN);
    if (pooled) hipLaunchKernelGGL((sp_dgrad_kernel<Net, BN, true>), grid, dim3(256), 0, st, gs, xs, wp, B, h, w, Cg, Cx, dx);
    else hipLaunchKernelGGL((sp_dgrad_kernel<Net, BN, false>), grid, dim3(256), 0, st, gs, xs, wp, B, h, w, Cg, Cx, dx);
}

// The backward of the nine 3x3 layers below g_hidden, top down, for either network (`net`: see the head of this file).  grads is the
// natural-order twin of the packed layout (w1a [64][9], b1a, w[j] [Cout][Cin][9], b[j]; the bias slots are written with Net::kBias only);
// layer_grads, if not null, receives what every layer's kernels saw as the gradient of its pre-activation output.
template <class Net, class Host>
void backward_layers(Host& net, int B, int H, int W, const float* image, const float* packed_grad, const float* g, int first_layer, float* grads,
                     float* layer_grads, float* ws, const BackwardWs& Wk, hipStream_t st) {
    const SpLayout L = sp_layout();
    float* part = ws + Wk.part;
    for (int j = SP_LAYERS - 1; j >= 0 && j + 1 >= first_layer; --j) {
        int h, w;
        layer_dims(j, H, W, h, w);
        const int Cin = kCin[j], Cout = kCout[j];
        const typename Net::Grad gs = net.grad(j + 1, g, h, w);
        const typename Net::In xs = net.input(j);
        const Split sp = wgrad_split(B, h, w, Cin, Cout);
        const int64_t nw = (int64_t)Cout * Cin * 9;
        float* part_b = part + (int64_t)sp.S * nw;
        const dim3 grid(sp.S, (Cin / 32) * (Cout / 32));
        bool inpool = false;                         // a pooled layer's input is never pooled (a-layers sit between)
        if constexpr (Net::kPoolOnLoad) inpool = j > 0 && kPooled[j - 1];
        if (kPooled[j]) {
            hipLaunchKernelGGL((sp_wgrad_kernel<Net, true, false>), grid, dim3(256), 0, st, gs, xs, B, h, w, Cin, Cout, sp.tiles_per, part, part_b);
        } else if (inpool) {
            if constexpr (Net::kPoolOnLoad)
                hipLaunchKernelGGL((sp_wgrad_kernel<Net, false, true>), grid, dim3(256), 0, st, gs, xs, B, h, w, Cin, Cout, sp.tiles_per, part, part_b);
        } else {
            hipLaunchKernelGGL((sp_wgrad_kernel<Net, false, false>), grid, dim3(256), 0, st, gs, xs, B, h, w, Cin, Cout, sp.tiles_per, part, part_b);
        }
        reduce_parts(part, sp.S, nw, grads + L.w[j], st);
        if constexpr (Net::kBias) reduce_parts(part_b, sp.S, Cout, grads + L.b[j], st);
        if (layer_grads) {
            int64_t off = Net::kDump1a ? (int64_t)B * H * W * 64 : 0;
            for (int i = 0; i < j; ++i) {
                int hi, wi;
                layer_dims(i, H, W, hi, wi);
                off += (int64_t)B * hi * wi * kCout[i];
            }
            grad_dump<Net>(gs, kPooled[j], B, h, w, Cout, layer_grads + off, st);
        }
        if (j < first_layer) break;                  // nothing below needs a gradient
        float* dx = ws + (j % 2 == 0 ? Wk.buf_even : Wk.buf_odd);
        const float* wp = packed_grad + dgrad_offset(j);
        // 128 output channels per workgroup only where the pixel tiles alone fill the chip: at coarse resolution (38 tiles at 480 x 640)
        // two workgroups of 64 channels halve the serial MFMA chain of a wave.  The sums per output are the same either way.
        const int tiles = conv_tiles(B, h, w);
        if (Cin == 64 || tiles < 512) dgrad<Net, 64>(gs, xs, kPooled[j], wp, B, h, w, Cout, Cin, dx, st);
        else dgrad<Net, 128>(gs, xs, kPooled[j], wp, B, h, w, Cout, Cin, dx, st);
        g = dx;
    }
    if (first_layer == 0) {
        const typename Net::Grad gs = net.grad(0, g, H, W);
        const int S1 = wgrad1a_splits(B, H, W);
        float* part_b = part + (int64_t)S1 * 64 * 9;
        hipLaunchKernelGGL(sp_wgrad1a_kernel<Net>, dim3(S1), dim3(256), 0, st, gs, image, B, H, W, SP_1A_PIX, part, part_b);
        reduce_parts(part, S1, 64 * 9, grads + L.w1a, st);
        if constexpr (Net::kBias) reduce_parts(part_b, S1, 64, grads + L.b1a, st);
        if (Net::kDump1a && layer_grads) grad_dump<Net>(gs, false, B, H, W, 64, layer_grads, st);
    }
}

}  // namespace

