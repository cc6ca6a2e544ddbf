// MegaDepth training pairs: the arithmetic of the reference's main-stage data items (data/megadepth_dataset.py:119-192
// MegaDepthPairsDataset.__getitem__, :203-282 MegaDepthPairsDatasetFeatures.__getitem__ and the collate data/megadepth_datamodule.py:105-166
// stack_keypoints_batch), which the reference runs with cv2 and numpy in its data-loader workers: grey, aspect-preserving resize of the
// image and of its depth map, crop to the target size, rescale and shift of K; for cached features the crop mask, the selection of
// num_keypoints keypoints and one depth value per keypoint.
//
//   resize_u8_kernel<C>        cv2.resize(INTER_LINEAR) on bytes, restricted to a destination window, equal-sized batch
//   resize_f32_kernel<NEAREST> the same for float maps ('linear' with unfused float32 arithmetic, or 'nearest')
//   md_image_kernel            all 2 B frames of a ragged batch in one launch from a device table: grey(taps) -> fixed-point resize -> / 255.f,
//                              only the crop window; thread (0, 0) of every frame's first workgroup row also writes the frame's K
//   md_depth_kernel<NEAREST>   the 2 B depth maps, same shape
//   md_features_kernel         one workgroup per image: crop mask, stable compaction or top-num_keypoints selection, gather, depth, K
//
// The arithmetic, once (tests/megadepth_ref.py restates it in numpy; the kernels are bit-identical to that):
//   taps      destination index d of an axis resized from src to dst:  scale = 1.0 / ((double)dst / src);  f = (float)((d + 0.5) scale - 0.5)
//             (every fp64 operation rounded on its own);  s = floor(f), f -= s;  s < 0 -> s = 0, f = 0;  s >= src - 1 -> s = src - 1, f = 0;
//             second tap min(s + 1, src - 1).
//   bytes     a1 = rint(f 2048), a0 = rint((1 - f) 2048) (half to even), likewise b0, b1 down the rows;  R = S[s] a0 + S[s + 1] a1 (int32);
//             out = (((b0 (R0 >> 4)) >> 16) + ((b1 (R1 >> 4)) >> 16) + 2) >> 2.  cv2's 11-bit scheme.
//   floats    R = S[s] (1 - f) + S[s + 1] f, out = R0 (1 - g) + R1 g: products and sums rounded separately (no fma).
//   nearest   s = min(floor(d (1.0 / ((double)dst / src))), src - 1) in fp64.
//   grey      (9798 R + 19235 G + 3735 B + 16384) >> 15 on the SOURCE taps (the reference converts before it resizes); one channel: the byte.
//   K         s_r K[r][c] with s_0 = (float)((double)resize_w / W), s_1 = (float)((double)resize_h / H), s_2 = 1, one float32 product, + 0.f
//             (the zero terms of the reference's 3 x 3 product turn a -0 into +0); then K[0][2] -= (float)x0, K[1][2] -= (float)y0.
//
// These are gathers bound by memory and launch latency.  Lanes run along x and every thread owns four adjacent destination pixels of two
// rows: the column taps and coefficients are computed once per thread, the stores of a wave are one contiguous 1 KiB segment (16 bytes per
// lane where the row length allows), and neighbouring lanes gather neighbouring source bytes, which L2 serves.
#include "og_block.h"

namespace {

constexpr int kPx = 4;                       // adjacent destination pixels per thread
constexpr int kLanesX = 64, kRowsY = 4;      // workgroup 64 x 4 threads
constexpr int kRowsPerThread = 2;            // rows y and y + kRowsY
constexpr int kTileW = kLanesX * kPx, kTileH = kRowsY * kRowsPerThread;
constexpr int kMaxSide = 32768, kMaxFrames = 65535;
constexpr int kMaxKeypoints = 8192;          // keypoints per image (keys in LDS)
constexpr int kMaxSelected = 4096;           // num_keypoints (source indices in LDS)

struct Geom {
    int H, W;        // source
    int rw, rh;      // resized
    int x0, y0;      // origin of the window in the resized image
};

__device__ __forceinline__ double axis_scale(int src, int dst) { return 1.0 / ((double)dst / (double)src); }

// taps and fraction of destination index d (0 <= d < dst); s0, s1 in [0, src)
__device__ __forceinline__ void linear_tap(int d, int src, double scale, int& s0, int& s1, float& f) {
#pragma clang fp contract(off)
    const float v = (float)(((double)d + 0.5) * scale - 0.5);
    const float fl = floorf(v);
    int s = (int)fl;
    f = v - fl;
    if (s < 0) { s = 0; f = 0.f; }
    if (s >= src - 1) { s = src - 1; f = 0.f; }
    s0 = s;
    s1 = min(s + 1, src - 1);
}

__device__ __forceinline__ int nearest_tap(int d, int src, double scale) {
#pragma clang fp contract(off)
    return min((int)floor((double)d * scale), src - 1);
}

__device__ __forceinline__ int coef(float f) { return (int)rintf(f * 2048.f); }

__device__ __forceinline__ int vertical_u8(int R0, int R1, int b0, int b1) { return (((b0 * (R0 >> 4)) >> 16) + ((b1 * (R1 >> 4)) >> 16) + 2) >> 2; }

// two products and a sum, each rounded on its own (HIP's default would contract them into an fma)
__device__ __forceinline__ float lerp_f32(float s0, float s1, float f) {
#pragma clang fp contract(off)
    const float a = s0 * (1.f - f), b = s1 * f;
    return a + b;
}

__device__ __forceinline__ int grey_at(const uint8_t* __restrict__ img, int64_t pixel, int C) {
    if (C == 1) return img[pixel];
    const uint8_t* p = img + pixel * 3;
    return (9798 * p[0] + 19235 * p[1] + 3735 * p[2] + 16384) >> 15;
}

// The column taps of the kPx pixels of this thread.  A pixel past the window's end takes the window's last column: it reads inside the
// source and is never stored.
struct Cols {
    int s0[kPx], s1[kPx];
    float f[kPx];
};
__device__ __forceinline__ Cols linear_cols(const Geom& g, int x, int w) {
    Cols c;
    const double sc = axis_scale(g.W, g.rw);
#pragma unroll
    for (int j = 0; j < kPx; ++j) linear_tap(g.x0 + min(x + j, w - 1), g.W, sc, c.s0[j], c.s1[j], c.f[j]);
    return c;
}

// four floats of one destination row: 16 bytes at once where every row starts on a 16-byte boundary (w % 4 == 0, base aligned)
__device__ __forceinline__ void store_px(float* __restrict__ row, int x, int w, const float (&v)[kPx]) {
    if ((w & 3) == 0) {
        f32x4 q = {v[0], v[1], v[2], v[3]};
        *(f32x4*)(row + x) = q;
    } else {
#pragma unroll
        for (int j = 0; j < kPx; ++j)
            if (x + j < w) row[x + j] = v[j];
    }
}

// ---- equal-sized batches: the primitives ----
template <int C>
__global__ __launch_bounds__(kLanesX* kRowsY) void resize_u8_kernel(Geom g, const uint8_t* __restrict__ src, int w, int h, uint8_t* __restrict__ dst) {
    const int x = (blockIdx.x * kLanesX + threadIdx.x) * kPx;
    if (x >= w) return;
    const uint8_t* img = src + (int64_t)blockIdx.z * g.H * g.W * C;
    const Cols c = linear_cols(g, x, w);
    const double sy = axis_scale(g.H, g.rh);
#pragma unroll
    for (int r = 0; r < kRowsPerThread; ++r) {
        const int y = blockIdx.y * kTileH + r * kRowsY + threadIdx.y;
        if (y >= h) continue;
        int t0, t1;
        float fy;
        linear_tap(g.y0 + y, g.H, sy, t0, t1, fy);
        const int b0 = coef(1.f - fy), b1 = coef(fy);
        const uint8_t *r0 = img + (int64_t)t0 * g.W * C, *r1 = img + (int64_t)t1 * g.W * C;
        uint8_t* o = dst + (((int64_t)blockIdx.z * h + y) * w + x) * C;
#pragma unroll
        for (int j = 0; j < kPx; ++j) {
            if (x + j >= w) break;
            const int a0 = coef(1.f - c.f[j]), a1 = coef(c.f[j]);
#pragma unroll
            for (int k = 0; k < C; ++k) {
                const int R0 = r0[c.s0[j] * C + k] * a0 + r0[c.s1[j] * C + k] * a1;
                const int R1 = r1[c.s0[j] * C + k] * a0 + r1[c.s1[j] * C + k] * a1;
                o[j * C + k] = (uint8_t)vertical_u8(R0, R1, b0, b1);
            }
        }
    }
}

// one destination row of a float map: kPx values of row y of the window
template <bool NEAREST>
__device__ __forceinline__ void depth_row(const Geom& g, const float* __restrict__ map, const Cols& c, const int (&n)[kPx], double sy, int y, float (&v)[kPx]) {
    if constexpr (NEAREST) {
        const float* r0 = map + (int64_t)nearest_tap(g.y0 + y, g.H, sy) * g.W;
#pragma unroll
        for (int j = 0; j < kPx; ++j) v[j] = r0[n[j]];
    } else {
        int t0, t1;
        float fy;
        linear_tap(g.y0 + y, g.H, sy, t0, t1, fy);
        const float *r0 = map + (int64_t)t0 * g.W, *r1 = map + (int64_t)t1 * g.W;
#pragma unroll
        for (int j = 0; j < kPx; ++j) v[j] = lerp_f32(lerp_f32(r0[c.s0[j]], r0[c.s1[j]], c.f[j]), lerp_f32(r1[c.s0[j]], r1[c.s1[j]], c.f[j]), fy);
    }
}

// the window (w x h at g.x0, g.y0) of one resized float map -> out [h][w]
template <bool NEAREST>
__device__ __forceinline__ void depth_window(const Geom& g, const float* __restrict__ map, int w, int h, float* __restrict__ out) {
    const int x = (blockIdx.x * kLanesX + threadIdx.x) * kPx;
    if (x >= w) return;
    Cols c = {};
    int n[kPx] = {};
    if constexpr (NEAREST) {
        const double sc = axis_scale(g.W, g.rw);
#pragma unroll
        for (int j = 0; j < kPx; ++j) n[j] = nearest_tap(g.x0 + min(x + j, w - 1), g.W, sc);
    } else {
        c = linear_cols(g, x, w);
    }
    const double sy = axis_scale(g.H, g.rh);
#pragma unroll
    for (int r = 0; r < kRowsPerThread; ++r) {
        const int y = blockIdx.y * kTileH + r * kRowsY + threadIdx.y;
        if (y >= h) continue;
        float v[kPx];
        depth_row<NEAREST>(g, map, c, n, sy, y, v);
        store_px(out + (int64_t)y * w, x, w, v);
    }
}

template <bool NEAREST>
__global__ __launch_bounds__(kLanesX* kRowsY) void resize_f32_kernel(Geom g, const float* __restrict__ src, int w, int h, float* __restrict__ dst) {
    depth_window<NEAREST>(g, src + (int64_t)blockIdx.z * g.H * g.W, w, h, dst + (int64_t)blockIdx.z * h * w);
}

// ---- ragged batches: one table entry per frame ----
__device__ __forceinline__ Geom geom_of(const og_md_frame& e) { return Geom{e.H, e.W, e.resize_w, e.resize_h, e.x0, e.y0}; }

__device__ __forceinline__ void write_K(const float* __restrict__ K, int W, int H, int rw, int rh, float sx, float sy, float* __restrict__ out, int t) {
#pragma clang fp contract(off)
    const int r = t / 3;
    const float s = r == 0 ? (float)((double)rw / (double)W) : r == 1 ? (float)((double)rh / (double)H) : 1.f;
    float v = s * K[t];
    v = v + 0.f;
    if (t == 2) v = v - sx;
    if (t == 5) v = v - sy;
    out[t] = v;
}

__global__ __launch_bounds__(kLanesX* kRowsY) void md_image_kernel(const og_md_frame* __restrict__ table, int w, int h, float* __restrict__ images,
                                                                   float* __restrict__ K_out) {
    const og_md_frame e = table[blockIdx.z];
    const Geom g = geom_of(e);
    if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.y == 0 && threadIdx.x < 9)
        write_K(e.K, e.W, e.H, e.resize_w, e.resize_h, (float)e.x0, (float)e.y0, K_out + (int64_t)blockIdx.z * 9, threadIdx.x);
    const int x = (blockIdx.x * kLanesX + threadIdx.x) * kPx;
    if (x >= w) return;
    const Cols c = linear_cols(g, x, w);
    const double sy = axis_scale(g.H, g.rh);
    float* out = images + (int64_t)blockIdx.z * h * w;
#pragma unroll
    for (int r = 0; r < kRowsPerThread; ++r) {
        const int y = blockIdx.y * kTileH + r * kRowsY + threadIdx.y;
        if (y >= h) continue;
        int t0, t1;
        float fy;
        linear_tap(g.y0 + y, g.H, sy, t0, t1, fy);
        const int b0 = coef(1.f - fy), b1 = coef(fy);
        const int64_t r0 = (int64_t)t0 * g.W, r1 = (int64_t)t1 * g.W;
        float v[kPx];
#pragma unroll
        for (int j = 0; j < kPx; ++j) {
            const int a0 = coef(1.f - c.f[j]), a1 = coef(c.f[j]);
            const int R0 = grey_at(e.image, r0 + c.s0[j], e.C) * a0 + grey_at(e.image, r0 + c.s1[j], e.C) * a1;
            const int R1 = grey_at(e.image, r1 + c.s0[j], e.C) * a0 + grey_at(e.image, r1 + c.s1[j], e.C) * a1;
            v[j] = (float)vertical_u8(R0, R1, b0, b1) / 255.f;
        }
        store_px(out + (int64_t)y * w, x, w, v);
    }
}

template <bool NEAREST>
__global__ __launch_bounds__(kLanesX* kRowsY) void md_depth_kernel(const og_md_frame* __restrict__ table, int w, int h, float* __restrict__ depths) {
    const og_md_frame e = table[blockIdx.z];
    depth_window<NEAREST>(geom_of(e), e.depth, w, h, depths + (int64_t)blockIdx.z * h * w);
}

// ---- cached features: one workgroup of 256 threads per image ----
__global__ __launch_bounds__(256) void md_features_kernel(const og_md_features* __restrict__ table, int tw, int th, int k, int D, float* __restrict__ lafs_out,
                                                          float* __restrict__ scores_out, float* __restrict__ desc_out, float* __restrict__ depth_out,
                                                          float* __restrict__ K_out) {
    __shared__ float key[kMaxKeypoints];
    __shared__ uint32_t inside[kMaxKeypoints / 32];      // bit i: keypoint i lies in the crop
    __shared__ int source[kMaxSelected];                 // output slot -> keypoint, -1: padding
    __shared__ int wsum[4];
    const og_md_features e = table[blockIdx.x];
    const int tid = threadIdx.x, n = e.n, axis = e.axis;
    const float* keys = e.keys ? e.keys : e.scores;
    const float lo = (float)e.start, hi = (float)(e.start + (axis == 0 ? tw : th));
    if (tid < 9) write_K(e.K, e.orig_w, e.orig_h, e.image_w, e.image_h, axis == 0 ? lo : 0.f, axis == 1 ? lo : 0.f, K_out + (int64_t)blockIdx.x * 9, tid);
    for (int p = tid; p < k; p += 256) source[p] = -1;
    // the crop mask, and the stable compaction that is the answer when at most k keypoints survive
    int survivors = 0;
    for (int c0 = 0; c0 < n; c0 += 256) {
        const int i = c0 + tid;
        bool flag = false;
        if (i < n) {
            key[i] = keys[i];
            const float c = axis >= 0 ? e.lafs[(int64_t)i * 6 + axis * 3 + 2] : 0.f;
            flag = axis < 0 || (c >= lo && c < hi);
        }
        __syncthreads();                                 // wsum of the previous round has been read; source[] is initialised
        int total;
        const int rank = survivors + block_rank_of(flag, wsum, total);
        const unsigned long long bal = __ballot(flag);
        if ((tid & 63) == 0) {
            inside[(c0 + tid) >> 5] = (uint32_t)bal;
            inside[((c0 + tid) >> 5) + 1] = (uint32_t)(bal >> 32);
        }
        if (flag && rank < k) source[rank] = i;
        survivors += total;
    }
    __syncthreads();
    if (survivors > k) {
        // the k largest keys in descending order, the lower index first on ties: the rank of a survivor is the number of survivors before it
        for (int i = tid; i < n; i += 256) {
            if (!((inside[i >> 5] >> (i & 31)) & 1u)) continue;
            const float ki = key[i];
            int rank = 0;
            for (int j = 0; j < n; ++j) {
                const float kj = key[j];
                const bool in = (inside[j >> 5] >> (j & 31)) & 1u;
                rank += in && (kj > ki || (kj == ki && j < i));
            }
            if (rank < k) source[rank] = i;
        }
        __syncthreads();
    }
    // gather; padding slots are zero
    const int64_t base = (int64_t)blockIdx.x * k;
    const int cw = axis == 0 ? tw : e.image_w, ch = axis == 1 ? th : e.image_h;      // the cropped depth map of the reference
    const double scx = axis_scale(e.depth_w, e.image_w), scy = axis_scale(e.depth_h, e.image_h);
    for (int p = tid; p < k; p += 256) {
        const int i = source[p];
        float l[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, s = 0.f, d = 0.f;
        if (i >= 0) {
#pragma unroll
            for (int q = 0; q < 6; ++q) l[q] = e.lafs[(int64_t)i * 6 + q];
            if (axis == 0) l[2] = l[2] - lo;
            if (axis == 1) l[5] = l[5] - lo;
            s = e.scores[i];
            const float x = l[2], y = l[5];
            if (x > -1.f && y > -1.f && x < (float)cw && y < (float)ch) {         // a NaN fails; (int) truncates towards zero
                const int rx = (int)x + (axis == 0 ? e.start : 0), ry = (int)y + (axis == 1 ? e.start : 0);
                d = e.depth[(int64_t)nearest_tap(ry, e.depth_h, scy) * e.depth_w + nearest_tap(rx, e.depth_w, scx)];
            }
        }
#pragma unroll
        for (int q = 0; q < 6; ++q) lafs_out[(base + p) * 6 + q] = l[q];
        scores_out[base + p] = s;
        depth_out[base + p] = d;
    }
    for (int64_t t = tid; t < (int64_t)k * D; t += 256) {
        const int p = (int)(t / D), c = (int)(t % D);
        const int i = source[p];
        desc_out[base * D + t] = i >= 0 ? e.descriptors[(int64_t)i * D + c] : 0.f;
    }
}

bool resize_ok(int32_t B, int32_t H, int32_t W, int32_t dw, int32_t dh, int32_t x0, int32_t y0, int32_t w, int32_t h) {
    return B >= 1 && B <= kMaxFrames && H >= 1 && H <= kMaxSide && W >= 1 && W <= kMaxSide && dw >= 1 && dw <= kMaxSide && dh >= 1 && dh <= kMaxSide &&
           w >= 1 && h >= 1 && x0 >= 0 && y0 >= 0 && x0 <= dw - w && y0 <= dh - h;
}
dim3 window_grid(int w, int h, int B) { return dim3((w + kTileW - 1) / kTileW, (h + kTileH - 1) / kTileH, B); }

}  // namespace

extern "C" int og_resize_linear_u8(int32_t batch, int32_t H, int32_t W, int32_t C, const uint8_t* src, int32_t dw, int32_t dh, int32_t x0, int32_t y0,
                                   int32_t w, int32_t h, uint8_t* dst, void* stream) {
    og_clear_status();
    if (!src || !dst) return OG_E_INVALID;
    if (!resize_ok(batch, H, W, dw, dh, x0, y0, w, h) || (C != 1 && C != 3)) return OG_E_SHAPE;
    const Geom g{H, W, dw, dh, x0, y0};
    const dim3 grid = window_grid(w, h, batch), block(kLanesX, kRowsY);
    if (C == 1) hipLaunchKernelGGL(resize_u8_kernel<1>, grid, block, 0, (hipStream_t)stream, g, src, w, h, dst);
    else hipLaunchKernelGGL(resize_u8_kernel<3>, grid, block, 0, (hipStream_t)stream, g, src, w, h, dst);
    return og_launch_status();
}

extern "C" int og_resize_f32(int32_t batch, int32_t H, int32_t W, const float* src, int32_t dw, int32_t dh, int32_t nearest, int32_t x0, int32_t y0,
                             int32_t w, int32_t h, float* dst, void* stream) {
    og_clear_status();
    if (!src || !dst) return OG_E_INVALID;
    if (!resize_ok(batch, H, W, dw, dh, x0, y0, w, h)) return OG_E_SHAPE;
    if (nearest != 0 && nearest != 1) return OG_E_FLAG;
    if ((uintptr_t)src & 3 || (uintptr_t)dst & 15) return OG_E_ALIGN;
    const Geom g{H, W, dw, dh, x0, y0};
    const dim3 grid = window_grid(w, h, batch), block(kLanesX, kRowsY);
    if (nearest) hipLaunchKernelGGL(resize_f32_kernel<true>, grid, block, 0, (hipStream_t)stream, g, src, w, h, dst);
    else hipLaunchKernelGGL(resize_f32_kernel<false>, grid, block, 0, (hipStream_t)stream, g, src, w, h, dst);
    return og_launch_status();
}

extern "C" int og_megadepth_pairs(int32_t frames, int32_t tw, int32_t th, const og_md_frame* table_host, const og_md_frame* table_dev, float* images,
                                  float* depths, float* K_out, int32_t depth_nearest, void* stream) {
    og_clear_status();
    if (!table_host || !table_dev || !images || !depths || !K_out) return OG_E_INVALID;
    if (frames < 1 || frames > kMaxFrames || tw < 1 || th < 1) return OG_E_SHAPE;
    if (depth_nearest != 0 && depth_nearest != 1) return OG_E_FLAG;
    if (((uintptr_t)images | (uintptr_t)depths) & 15 || (uintptr_t)K_out & 3 || (uintptr_t)table_dev & 7) return OG_E_ALIGN;
    for (int i = 0; i < frames; ++i) {
        const og_md_frame& e = table_host[i];
        if (!e.image || !e.depth || !e.K) return OG_E_INVALID;
        if (!resize_ok(1, e.H, e.W, e.resize_w, e.resize_h, e.x0, e.y0, tw, th) || (e.C != 1 && e.C != 3)) return OG_E_SHAPE;
        if (((uintptr_t)e.depth | (uintptr_t)e.K) & 3) return OG_E_ALIGN;
    }
    const dim3 grid = window_grid(tw, th, frames), block(kLanesX, kRowsY);
    hipLaunchKernelGGL(md_image_kernel, grid, block, 0, (hipStream_t)stream, table_dev, tw, th, images, K_out);
    if (depth_nearest) hipLaunchKernelGGL(md_depth_kernel<true>, grid, block, 0, (hipStream_t)stream, table_dev, tw, th, depths);
    else hipLaunchKernelGGL(md_depth_kernel<false>, grid, block, 0, (hipStream_t)stream, table_dev, tw, th, depths);
    return og_launch_status();
}

extern "C" int og_megadepth_features(int32_t images, int32_t tw, int32_t th, int32_t num_keypoints, int32_t desc_dim, const og_md_features* table_host,
                                     const og_md_features* table_dev, float* lafs, float* scores, float* descriptors, float* depth, float* K_out,
                                     void* stream) {
    og_clear_status();
    if (!table_host || !table_dev || !lafs || !scores || !descriptors || !depth || !K_out) return OG_E_INVALID;
    if (images < 1 || images > kMaxFrames || tw < 1 || th < 1 || tw > kMaxSide || th > kMaxSide || num_keypoints < 1 || num_keypoints > kMaxSelected ||
        desc_dim < 1 || desc_dim > 65536)
        return OG_E_SHAPE;
    if (((uintptr_t)lafs | (uintptr_t)scores | (uintptr_t)descriptors | (uintptr_t)depth | (uintptr_t)K_out) & 3 || (uintptr_t)table_dev & 7) return OG_E_ALIGN;
    for (int i = 0; i < images; ++i) {
        const og_md_features& e = table_host[i];
        if (!e.depth || !e.K || (e.n > 0 && (!e.lafs || !e.scores || !e.descriptors))) return OG_E_INVALID;
        if (e.n < 0 || e.n > kMaxKeypoints) return OG_E_SHAPE;
        for (int32_t v : {e.image_w, e.image_h, e.orig_w, e.orig_h, e.depth_w, e.depth_h})
            if (v < 1 || v > kMaxSide) return OG_E_SHAPE;
        if (e.axis < -1 || e.axis > 1 || e.start < 0 || (e.axis < 0 && e.start != 0)) return OG_E_SHAPE;
        if ((e.axis == 0 && e.start > e.image_w - tw) || (e.axis == 1 && e.start > e.image_h - th)) return OG_E_SHAPE;
        if (((uintptr_t)e.lafs | (uintptr_t)e.scores | (uintptr_t)e.descriptors | (uintptr_t)e.keys | (uintptr_t)e.depth | (uintptr_t)e.K) & 3) return OG_E_ALIGN;
    }
    hipLaunchKernelGGL(md_features_kernel, dim3(images), dim3(256), 0, (hipStream_t)stream, table_dev, tw, th, num_keypoints, desc_dim, lafs, scores, descriptors,
                       depth, K_out);
    return og_launch_status();
}
