// weak_color_aug: the photometric augmentation of the reference's online training step (models/matching_module.py:55-74 augment,
// utils/augmentations.py: kornia RandomEqualize, RandomSharpness, RandomSolarize, RandomGaussianNoise), which kornia runs as dozens of small
// launches with host synchronisations inside equalize.  Here: three launches, no synchronisation, one flag word and five scalars per sample.
//
//   coloraug_hist_kernel    grid (blocks per plane, C, B): the 256-bin histogram of kHistPixels pixels, one private histogram per wave in LDS
//                           (integer LDS atomics), merged per block and written with plain stores: partial[plane][block][256]
//   coloraug_lut_kernel     grid (C, B), 256 threads: the partials summed in block order, the last non-empty bin, step, the prefix sum
//                           (og_block.h), lut[plane][256] = the final floats k / 255 and the step == 0 marker
//   coloraug_apply_kernel   one kTileX x kTileY tile with a one-pixel halo per workgroup: the equalized values in LDS (LUT applied on load),
//                           then stencil, blend, solarize, noise; a thread owns four pixels of a row and stores them as one float4 where the
//                           address allows
// Planes of samples without the equalize flag leave the first two kernels at once; nothing waits on another workgroup; there is no float
// atomic, so every result is bit-identical from run to run and independent of the batch.
//
// The arithmetic, once (tests/coloraug_ref.py restates it in numpy; the kernels are bit-identical to that in everything but the noise, whose
// logf / cosf are the library's).  float32, every operation rounded on its own, true divisions.  The kernels are compiled under `#pragma clang fp
// contract(off)` with plain operators: the __fmul_rn / __fadd_rn of the HIP headers are inline functions compiled under the command line's
// contraction mode and fuse after inlining.  With the pragma the code equals that of -ffp-contract=off but for the compiler's own expansion of logf.
//   equalize   v = x * 255;  q = (v * 256) / 255;  bin = q >= 255 ? 255 : q >= 0 ? (int)q : 0 (NaN: 0);  idx likewise from v.
//              h = histogram of bin over the plane, N = H W;  step = (N - h[last non-empty bin]) / 255 (integers);
//              step == 0: y = v / 255;  else lut[k] = min(255, (sum_{j < k} h[j] + step / 2) / step), y = (float)lut[idx] / 255.
//   sharpness  interior pixels (0 < x < W - 1, 0 < y < H - 1): blur = sum of the nine taps in row-major order, acc = w p00, acc = acc + w p01,
//              ..., w = 1/13 (float), the centre 5/13 (float), products and sums rounded separately; blur = clamp(blur, 0, 1);
//              f == 0: blur;  f == 1: in;  else r = blur + (in - blur) f, clamped to [0, 1] unless 0 < f < 1.  Border pixels keep the input.
//   solarize   t = clamp(x + addition, 0, 1);  out = t < threshold ? t : 1 - t.
//   noise      i = (c H + y) W + x;  h = mix64(mix64(seed) + i);  u1 = ((h >> 40) + 1) 2^-24;  u2 = ((h >> 16) & 0xFFFFFF) 2^-24;
//              z = sqrtf(-2 logf(u1)) cosf(6.2831855f u2);  out = x + (mean + std z).
// clamp(t, 0, 1) is t < 0 ? 0 : t > 1 ? 1 : t: a NaN stays a NaN.
#include "og_ransac.h"      // mix64; og_block.h: the scan

namespace {

constexpr int kHistThreads = 256;
constexpr int kHistPixels = 8192;                 // pixels of a plane per histogram block
constexpr int kTileX = 64, kTileY = 16;           // the apply kernel's tile; 16 x 16 threads of four pixels
constexpr int kApplyThreads = (kTileX / 4) * kTileY;
constexpr int kLutStride = 256;

enum { kEqualize = 1, kSharpness = 2, kSolarize = 4, kNoise = 8 };

__device__ __forceinline__ int to_byte(float q) { return q >= 255.f ? 255 : (q >= 0.f ? (int)q : 0); }   // a NaN: 0

__device__ __forceinline__ float clamp01(float t) { return t < 0.f ? 0.f : (t > 1.f ? 1.f : t); }

__global__ __launch_bounds__(kHistThreads) void coloraug_hist_kernel(int64_t N, int nblk, const float* __restrict__ src, const int32_t* __restrict__ flags,
                                                                     uint32_t* __restrict__ partial) {
#pragma clang fp contract(off)
    const int b = blockIdx.z, c = blockIdx.y, C = gridDim.y;
    if (!(flags[b] & kEqualize)) return;                                // uniform: before any barrier
    __shared__ uint32_t h[4][256];
    const int tid = threadIdx.x, wave = tid >> 6;
#pragma unroll
    for (int w = 0; w < 4; ++w) h[w][tid] = 0u;
    __syncthreads();
    const int64_t plane = (int64_t)b * C + c;
    const float* p = src + plane * N;
    const int64_t i0 = (int64_t)blockIdx.x * kHistPixels;
    const int64_t i1 = i0 + kHistPixels < N ? i0 + kHistPixels : N;
#pragma unroll 8
    for (int64_t i = i0 + tid; i < i1; i += kHistThreads) {
        const float v = p[i] * 255.f;
        const float q = (v * 256.f) / 255.f;
        atomicAdd(&h[wave][to_byte(q)], 1u);
    }
    __syncthreads();
    partial[(plane * nblk + blockIdx.x) * 256 + tid] = ((h[0][tid] + h[1][tid]) + h[2][tid]) + h[3][tid];
}

__global__ __launch_bounds__(256) void coloraug_lut_kernel(int64_t N, int nblk, const int32_t* __restrict__ flags, const uint32_t* __restrict__ partial,
                                                           float* __restrict__ lut, int32_t* __restrict__ step0) {
    const int b = blockIdx.y, c = blockIdx.x, C = gridDim.x;
    if (!(flags[b] & kEqualize)) return;
    __shared__ int32_t a[256];
    __shared__ int32_t last[4];
    __shared__ int32_t total;
    const int tid = threadIdx.x;
    const int64_t plane = (int64_t)b * C + c;
    const uint32_t* p = partial + plane * nblk * 256 + tid;
    uint32_t cnt = 0u;
    for (int k = 0; k < nblk; ++k) cnt += p[(int64_t)k * 256];
    a[tid] = (int32_t)cnt;                                               // N <= 2^30
    int hi = cnt ? tid : -1;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) hi = max(hi, __shfl_xor(hi, o, 64));
    if ((tid & 63) == 0) last[tid >> 6] = hi;
    __syncthreads();
    hi = max(max(last[0], last[1]), max(last[2], last[3]));              // N >= 1: some bin is not empty
    const int32_t step = ((int32_t)N - a[hi]) / 255;
    __syncthreads();                                                     // a[hi] is read before the scan overwrites it
    block_exclusive_scan_inplace(a, 256, &total);                        // thread t owns entry t alone
    if (step == 0) {
        if (tid == 0) step0[plane] = 1;
        return;
    }
    if (tid == 0) step0[plane] = 0;
    const int32_t k = min(255, (a[tid] + step / 2) / step);
    lut[plane * kLutStride + tid] = (float)k / 255.f;
}

__global__ __launch_bounds__(kApplyThreads) void coloraug_apply_kernel(int H, int W, int tiles_x, const float* __restrict__ src, float* __restrict__ dst,
                                                                       const int32_t* __restrict__ flags, const float* __restrict__ scalars,
                                                                       const int64_t* __restrict__ seeds, const float* __restrict__ lut,
                                                                       const int32_t* __restrict__ step0) {
#pragma clang fp contract(off)
    __shared__ float tile[kTileY + 2][kTileX + 2];
    __shared__ float lds_lut[256];
    const int b = blockIdx.z, c = blockIdx.y, C = gridDim.y;
    const int tx = blockIdx.x % tiles_x, ty = blockIdx.x / tiles_x;
    const int x0 = tx * kTileX, y0 = ty * kTileY;
    const int tid = threadIdx.x;
    const int fl = flags[b];
    const int64_t plane = (int64_t)b * C + c;
    const float* p = src + plane * H * W;
    const bool eq = fl & kEqualize;
    const bool direct = eq && step0[plane] != 0;                          // step == 0: v / 255, no table
    if (eq && !direct) {
        for (int k = tid; k < 256; k += kApplyThreads) lds_lut[k] = lut[plane * kLutStride + k];
        __syncthreads();
    }
    for (int k = tid; k < (kTileY + 2) * (kTileX + 2); k += kApplyThreads) {
        const int ly = k / (kTileX + 2), lx = k - ly * (kTileX + 2);
        const int y = y0 + ly - 1, x = x0 + lx - 1;
        float e = 0.f;                                                    // outside the image: never used, border pixels keep the input
        if (y >= 0 && y < H && x >= 0 && x < W) {
            e = p[(int64_t)y * W + x];
            if (eq) {
                const float v = e * 255.f;
                e = direct ? v / 255.f : lds_lut[to_byte(v)];
            }
        }
        tile[ly][lx] = e;
    }
    __syncthreads();
    const int ly = tid / (kTileX / 4), lx = (tid % (kTileX / 4)) * 4;
    const int y = y0 + ly, xa = x0 + lx;
    if (y >= H || xa >= W) return;
    const float* s = scalars + (int64_t)b * 5;
    const float factor = s[0], threshold = s[1], addition = s[2], mean = s[3], stddev = s[4];
    const uint64_t base = mix64((uint64_t)seeds[b]) + (uint64_t)(((int64_t)c * H + y) * W);
    const float w1 = 1.f / 13.f, w5 = 5.f / 13.f;
    float out[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int x = xa + j;
        const int cy = ly + 1, cx = lx + j + 1;
        float v = tile[cy][cx];
        if ((fl & kSharpness) && x > 0 && x < W - 1 && y > 0 && y < H - 1) {
            float acc = w1 * tile[cy - 1][cx - 1];
            acc = acc + w1 * tile[cy - 1][cx];
            acc = acc + w1 * tile[cy - 1][cx + 1];
            acc = acc + w1 * tile[cy][cx - 1];
            acc = acc + w5 * v;
            acc = acc + w1 * tile[cy][cx + 1];
            acc = acc + w1 * tile[cy + 1][cx - 1];
            acc = acc + w1 * tile[cy + 1][cx];
            acc = acc + w1 * tile[cy + 1][cx + 1];
            const float blur = clamp01(acc);
            if (factor == 0.f) v = blur;
            else if (factor != 1.f) {
                const float r = blur + (v - blur) * factor;
                v = factor > 0.f && factor < 1.f ? r : clamp01(r);
            }
        }
        if (fl & kSolarize) {
            const float t = clamp01(v + addition);
            v = t < threshold ? t : 1.f - t;
        }
        if (fl & kNoise) {
            const uint64_t hsh = mix64(base + (uint64_t)x);
            const float u1 = (float)((uint32_t)(hsh >> 40) + 1u) * 5.9604644775390625e-8f;            // 2^-24, exact
            const float u2 = (float)((uint32_t)(hsh >> 16) & 0xFFFFFFu) * 5.9604644775390625e-8f;
            const float z = sqrtf(-2.f * logf(u1)) * cosf(6.2831855f * u2);
            v = v + (mean + stddev * z);
        }
        out[j] = v;
    }
    float* o = dst + plane * H * W + (int64_t)y * W + xa;
    if (xa + 3 < W && ((uintptr_t)o & 15) == 0) {
        *reinterpret_cast<f32x4*>(o) = f32x4{out[0], out[1], out[2], out[3]};
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (xa + j < W) o[j] = out[j];
    }
}

bool frame_ok(int32_t B, int32_t C, int32_t H, int32_t W) {
    return B >= 1 && B <= 65535 && H >= 1 && H <= 32768 && W >= 1 && W <= 32768 && (C == 1 || C == 3);
}
int64_t hist_blocks(int64_t N) { return (N + kHistPixels - 1) / kHistPixels; }
// workspace: partial u32 [planes][blocks][256] | lut float [planes][256] | step0 int32 [planes]
int64_t partial_bytes(int64_t planes, int64_t N) { return planes * hist_blocks(N) * 256 * 4; }

}  // namespace

extern "C" size_t og_color_aug_workspace_bytes(int32_t batch, int32_t C, int32_t H, int32_t W) {
    if (!frame_ok(batch, C, H, W)) return 0;
    const int64_t planes = (int64_t)batch * C, N = (int64_t)H * W;
    return (size_t)og_round_up(partial_bytes(planes, N) + planes * kLutStride * 4 + planes * 4, 256);
}

extern "C" int og_color_aug(int32_t batch, int32_t C, int32_t H, int32_t W, const float* src, float* dst, const int32_t* flags, const float* scalars,
                            const int64_t* seeds, void* workspace_dev, size_t workspace_bytes, void* stream) {
    og_clear_status();
    if (!src || !dst || !flags || !scalars || !seeds || !workspace_dev || (const float*)dst == src) return OG_E_INVALID;
    if (!frame_ok(batch, C, H, W) || workspace_bytes < og_color_aug_workspace_bytes(batch, C, H, W)) return OG_E_SHAPE;
    if (((uintptr_t)src | (uintptr_t)dst | (uintptr_t)flags | (uintptr_t)scalars | (uintptr_t)workspace_dev) & 3 || (uintptr_t)seeds & 7) return OG_E_ALIGN;
    hipStream_t st = (hipStream_t)stream;
    const int64_t planes = (int64_t)batch * C, N = (int64_t)H * W;
    const int nblk = (int)hist_blocks(N);
    uint32_t* partial = (uint32_t*)workspace_dev;
    float* lut = (float*)((char*)workspace_dev + partial_bytes(planes, N));
    int32_t* step0 = (int32_t*)(lut + planes * kLutStride);
    hipLaunchKernelGGL(coloraug_hist_kernel, dim3(nblk, C, batch), dim3(kHistThreads), 0, st, N, nblk, src, flags, partial);
    hipLaunchKernelGGL(coloraug_lut_kernel, dim3(C, batch), dim3(256), 0, st, N, nblk, flags, (const uint32_t*)partial, lut, step0);
    const int tiles_x = (W + kTileX - 1) / kTileX, tiles_y = (H + kTileY - 1) / kTileY;
    hipLaunchKernelGGL(coloraug_apply_kernel, dim3(tiles_x * tiles_y, C, batch), dim3(kApplyThreads), 0, st, H, W, tiles_x, src, dst, flags, scalars, seeds,
                       (const float*)lut, (const int32_t*)step0);
    return og_launch_status();
}
