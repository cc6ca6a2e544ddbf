// Homography training pairs: the arithmetic of the reference's self-supervised data items (data/oxford_paris_dataset.py:27-66
// OxfordParis1MDataset.__getitem__, data/megadepth_dataset.py:33-52 MegaDepthWarpingDataset.__getitem__), which the reference runs with
// cv2 in its data-loader workers: getPerspectiveTransform, warpPerspective, crop, grey, / 255.
//
//   perspective_transform_kernel   one thread per 8 x 8 system, the augmented matrix in LDS ([entry][thread]: no bank conflicts, no scratch)
//   pairs_solve_kernel             the same solver for both systems of an Oxford-Paris item (thread 2 b: H_warp, fp64; 2 b + 1: H_true, fp32)
//   warp_u8_kernel<C>              cv2.warpPerspective on a destination window, bytes out
//   pairs_kernel<C>                both views of every pair in one launch: grey(frame window) / 255, grey(warp window) / 255; the warped bytes
//                                  never leave registers
//
// The arithmetic, once (tests/pairs_ref.py restates it in numpy; the kernels are bit-identical to that):
//   solver    point i: row i = [x y 1 0 0 0 -xu -yu | u], row i + 4 = [0 0 0 x y 1 -xv -yv | v]; fp64 Gaussian elimination with partial
//             pivoting (the first largest |entry| of the column), a[i][j] -= (a[i][k] / a[k][k]) a[k][j], back substitution, M[2][2] = 1.
//             A pivot not above 1e-12 max|coefficient| (zero at the level of rounding) or a non-finite solution: M = 0.
//   inverse   Mi = adj(M) * (1 / det M), det by the first row; Mi = 0 when det == 0.  Once per image (thread 0 of every workgroup, 40 flops).
//   source    destination pixel (x, y) of the full frame:  Wd = (Mi20 x + Mi21 y) + Mi22;  s = Wd != 0 ? 32 / Wd : 0;
//             fX = ((Mi00 x + Mi01 y) + Mi02) s;  fY = ((Mi10 x + Mi11 y) + Mi12) s;  fX > INT_MAX -> INT_MAX, !(fX >= INT_MIN) -> INT_MIN;
//             X = rint(fX), Y = rint(fY) (half to even).  fp64, every operation rounded on its own (no contraction), a true division.
//   taps      sx = X >> 5, fx = X & 31, sy = Y >> 5, fy = Y & 31 (arithmetic shift); (sy, sx), (sy, sx + 1), (sy + 1, sx), (sy + 1, sx + 1); a tap
//             outside the source is 0.  Weights 32 (32 - fx)(32 - fy), 32 fx (32 - fy), 32 (32 - fx) fy, 32 fx fy: exact integers that sum to
//             32768, which is cv2's 15-bit bilinear table at its 1/32-pixel steps.
//   output    (sum w v + 16384) >> 15 per channel;  grey = (9798 R + 19235 G + 3735 B + 16384) >> 15 on the warped bytes;  float(grey) / 255.f.
// Everything after rint is integer arithmetic.
//
// Memory-bound: an output pixel gathers 4 C bytes and stores C bytes (warp) or reads 5 C bytes and stores 8 (pairs).  Lanes run along x, so the
// stores of a wave are one contiguous segment and neighbouring lanes gather neighbouring bytes; a workgroup is 64 x 4 pixels.
#include "og_common.h"

namespace {

constexpr int kSolveThreads = 64;
constexpr int kTileX = 64, kTileY = 4;

// 8 x 9 augmented system of thread `tid` in LDS: entry (r, c) at a[(r * 9 + c) * kSolveThreads + tid]
struct Sys {
    double* a;
    __device__ __forceinline__ double& operator()(int r, int c) const { return a[(r * 9 + c) * kSolveThreads]; }
};

// src -> dst of four points, M[9] (row-major); all arithmetic fp64, nothing contracted
__device__ void solve_perspective(const Sys A, const float (&sx)[4], const float (&sy)[4], const float (&dx)[4], const float (&dy)[4], double (&M)[9]) {
#pragma clang fp contract(off)
    double amax = 0.0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const double x = sx[i], y = sy[i], u = dx[i], v = dy[i];
        const double r0[9] = {x, y, 1.0, 0.0, 0.0, 0.0, -x * u, -y * u, u};
        const double r1[9] = {0.0, 0.0, 0.0, x, y, 1.0, -x * v, -y * v, v};
#pragma unroll
        for (int c = 0; c < 9; ++c) {
            A(i, c) = r0[c];
            A(i + 4, c) = r1[c];
            if (c < 8) amax = fmax(amax, fmax(fabs(r0[c]), fabs(r1[c])));
        }
    }
    const double tiny = 1e-12 * amax;
    bool ok = true;
    // fully unrolled: every LDS address but the pivot row's is a constant, so the reads of a stage go out together.  After a failed pivot
    // the remaining stages still run (on infinities and NaNs, harmlessly) and the result is discarded.
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        int p = k;
        double best = fabs(A(k, k));
#pragma unroll
        for (int i = k + 1; i < 8; ++i) {
            const double v = fabs(A(i, k));
            if (v > best) { best = v; p = i; }
        }
        if (!(best > tiny)) ok = false;
        if (p != k)
#pragma unroll
            for (int c = k; c < 9; ++c) {
                const double t = A(k, c);
                A(k, c) = A(p, c);
                A(p, c) = t;
            }
        const double piv = A(k, k);
#pragma unroll
        for (int i = k + 1; i < 8; ++i) {
            const double f = A(i, k) / piv;
#pragma unroll
            for (int c = k + 1; c < 9; ++c) A(i, c) = A(i, c) - f * A(k, c);
        }
    }
#pragma unroll
    for (int i = 7; i >= 0; --i) {
        double s = A(i, 8);
#pragma unroll
        for (int c = i + 1; c < 8; ++c) s = s - A(i, c) * A(c, 8);
        s = s / A(i, i);
        A(i, 8) = s;                                   // the solution replaces the right-hand side
        if (!(fabs(s) <= 1.79769313486231570815e308)) ok = false;
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) M[i] = ok ? A(i, 8) : 0.0;
    M[8] = ok ? 1.0 : 0.0;
}

__global__ __launch_bounds__(kSolveThreads) void perspective_transform_kernel(int B, const float* __restrict__ src, const float* __restrict__ dst,
                                                                              double* __restrict__ M) {
    __shared__ double lds[72 * kSolveThreads];
    const int b = blockIdx.x * kSolveThreads + threadIdx.x;
    if (b >= B) return;                                  // no barrier below
    float sx[4], sy[4], dx[4], dy[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        sx[i] = src[(int64_t)b * 8 + 2 * i]; sy[i] = src[(int64_t)b * 8 + 2 * i + 1];
        dx[i] = dst[(int64_t)b * 8 + 2 * i]; dy[i] = dst[(int64_t)b * 8 + 2 * i + 1];
    }
    double m[9];
    solve_perspective(Sys{lds + threadIdx.x}, sx, sy, dx, dy, m);
#pragma unroll
    for (int i = 0; i < 9; ++i) M[(int64_t)b * 9 + i] = m[i];
}

// thread t: pair t >> 1; even t the warp matrix (full-frame corners, fp64 out), odd t H_true (crop corners, fp32 out).  The corners and the
// sums corner + offset are float32, as the reference forms them before cv2 sees them.
__global__ __launch_bounds__(kSolveThreads) void pairs_solve_kernel(int B, int H, int W, int offset, const float* __restrict__ warp_offset,
                                                                    double* __restrict__ H_warp, float* __restrict__ H_true) {
    __shared__ double lds[72 * kSolveThreads];
    const int t = blockIdx.x * kSolveThreads + threadIdx.x;
    if (t >= 2 * B) return;
    const int b = t >> 1;
    const bool crop = t & 1;
    const float lo = crop ? 0.f : (float)offset;
    const float xhi = (float)(W - offset - 1) - (crop ? (float)offset : 0.f), yhi = (float)(H - offset - 1) - (crop ? (float)offset : 0.f);
    const float cx[4] = {lo, lo, xhi, xhi}, cy[4] = {lo, yhi, lo, yhi};
    float sx[4], sy[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        sx[i] = cx[i] + warp_offset[(int64_t)b * 8 + 2 * i];
        sy[i] = cy[i] + warp_offset[(int64_t)b * 8 + 2 * i + 1];
    }
    double m[9];
    solve_perspective(Sys{lds + threadIdx.x}, sx, sy, cx, cy, m);
#pragma unroll
    for (int i = 0; i < 9; ++i) {
        if (crop) H_true[(int64_t)b * 9 + i] = (float)m[i];
        else H_warp[(int64_t)b * 9 + i] = m[i];
    }
}

// Mi = adj(M) * (1 / det), zero for det == 0
__device__ __forceinline__ void invert3(const double* __restrict__ M, double* Mi) {
#pragma clang fp contract(off)
    const double a = M[0], b = M[1], c = M[2], d = M[3], e = M[4], f = M[5], g = M[6], h = M[7], i = M[8];
    const double c00 = e * i - f * h, c01 = f * g - d * i, c02 = d * h - e * g;
    const double det = (a * c00 + b * c01) + c * c02;
    const double id = det != 0.0 ? 1.0 / det : 0.0;
    Mi[0] = c00 * id; Mi[1] = (c * h - b * i) * id; Mi[2] = (b * f - c * e) * id;
    Mi[3] = c01 * id; Mi[4] = (a * i - c * g) * id; Mi[5] = (c * d - a * f) * id;
    Mi[6] = c02 * id; Mi[7] = (b * g - a * h) * id; Mi[8] = (a * e - b * d) * id;
}

// fixed-point source coordinates of destination pixel (x, y)
__device__ __forceinline__ void source_xy(const double* Mi, int x, int y, int& X, int& Y) {
#pragma clang fp contract(off)
    const double xd = (double)x, yd = (double)y;
    const double Wd = (Mi[6] * xd + Mi[7] * yd) + Mi[8];
    const double s = Wd != 0.0 ? 32.0 / Wd : 0.0;
    double fX = ((Mi[0] * xd + Mi[1] * yd) + Mi[2]) * s;
    double fY = ((Mi[3] * xd + Mi[4] * yd) + Mi[5]) * s;
    fX = fX > 2147483647.0 ? 2147483647.0 : fX;
    fX = fX >= -2147483648.0 ? fX : -2147483648.0;         // a NaN goes here
    fY = fY > 2147483647.0 ? 2147483647.0 : fY;
    fY = fY >= -2147483648.0 ? fY : -2147483648.0;
    X = (int)rint(fX);
    Y = (int)rint(fY);
}

// the bilinear sample of every channel at (X, Y) / 32 of image `img` [H][W][C]
template <int C>
__device__ __forceinline__ void sample(const uint8_t* __restrict__ img, int H, int W, int X, int Y, int (&out)[C]) {
    const int sx = X >> 5, fx = X & 31, sy = Y >> 5, fy = Y & 31;
    const int w00 = 32 * (32 - fx) * (32 - fy), w01 = 32 * fx * (32 - fy), w10 = 32 * (32 - fx) * fy, w11 = 32 * fx * fy;
    const bool x0 = sx >= 0 && sx < W, x1 = sx >= -1 && sx < W - 1;             // sx + 1 in [0, W)
    const bool y0 = sy >= 0 && sy < H, y1 = sy >= -1 && sy < H - 1;
    // the address of an outside tap is never formed from its coordinates: it reads pixel (0, 0) and is multiplied by 0
    const int64_t r0 = y0 ? (int64_t)sy * W : 0, r1 = y1 ? (int64_t)(sy + 1) * W : 0;
    const int64_t q0 = x0 ? sx : 0, q1 = x1 ? sx + 1 : 0;
    const uint8_t* p00 = img + (y0 && x0 ? (r0 + q0) * C : 0);
    const uint8_t* p01 = img + (y0 && x1 ? (r0 + q1) * C : 0);
    const uint8_t* p10 = img + (y1 && x0 ? (r1 + q0) * C : 0);
    const uint8_t* p11 = img + (y1 && x1 ? (r1 + q1) * C : 0);
    const int m00 = y0 && x0 ? w00 : 0, m01 = y0 && x1 ? w01 : 0, m10 = y1 && x0 ? w10 : 0, m11 = y1 && x1 ? w11 : 0;
#pragma unroll
    for (int c = 0; c < C; ++c) out[c] = (m00 * p00[c] + m01 * p01[c] + m10 * p10[c] + m11 * p11[c] + 16384) >> 15;
}

template <int C>
__device__ __forceinline__ int grey(const int (&v)[C]) {
    if constexpr (C == 1) return v[0];
    else return (9798 * v[0] + 19235 * v[1] + 3735 * v[2] + 16384) >> 15;
}

// thread 0 inverts the matrix of image blockIdx.z into LDS; returns after the barrier
__device__ __forceinline__ void workgroup_inverse(const double* __restrict__ M, double* mi) {
    if (threadIdx.x == 0 && threadIdx.y == 0) invert3(M + (int64_t)blockIdx.z * 9, mi);
    __syncthreads();
}

template <int C>
__global__ __launch_bounds__(kTileX* kTileY) void warp_u8_kernel(int H, int W, const uint8_t* __restrict__ src, const double* __restrict__ M, int x0,
                                                                 int y0, int w, int h, uint8_t* __restrict__ dst) {
    __shared__ double mi[9];
    workgroup_inverse(M, mi);
    const int x = blockIdx.x * kTileX + threadIdx.x, y = blockIdx.y * kTileY + threadIdx.y;
    if (x >= w || y >= h) return;
    const int b = blockIdx.z;
    int X, Y, v[C];
    source_xy(mi, x + x0, y + y0, X, Y);
    sample<C>(src + (int64_t)b * H * W * C, H, W, X, Y, v);
    uint8_t* o = dst + (((int64_t)b * h + y) * w + x) * C;
#pragma unroll
    for (int c = 0; c < C; ++c) o[c] = (uint8_t)v[c];
}

template <int C>
__global__ __launch_bounds__(kTileX* kTileY) void pairs_kernel(int H, int W, const uint8_t* __restrict__ frames, const double* __restrict__ M,
                                                               int offset, float* __restrict__ image0, float* __restrict__ image1) {
    __shared__ double mi[9];
    workgroup_inverse(M, mi);
    const int w = W - 2 * offset, h = H - 2 * offset;
    const int x = blockIdx.x * kTileX + threadIdx.x, y = blockIdx.y * kTileY + threadIdx.y;
    if (x >= w || y >= h) return;
    const int b = blockIdx.z;
    const uint8_t* img = frames + (int64_t)b * H * W * C;
    int X, Y, v0[C], v1[C];
    source_xy(mi, x + offset, y + offset, X, Y);
    sample<C>(img, H, W, X, Y, v1);
    const uint8_t* p = img + ((int64_t)(y + offset) * W + (x + offset)) * C;
#pragma unroll
    for (int c = 0; c < C; ++c) v0[c] = p[c];
    const int64_t o = ((int64_t)b * h + y) * w + x;
    image0[o] = (float)grey<C>(v0) / 255.f;
    image1[o] = (float)grey<C>(v1) / 255.f;
}

bool frame_ok(int32_t B, int32_t H, int32_t W, int32_t C) {
    return B >= 1 && B <= 65535 && H >= 1 && H <= 32768 && W >= 1 && W <= 32768 && (C == 1 || C == 3);
}
dim3 tiles(int w, int h, int B) { return dim3((w + kTileX - 1) / kTileX, (h + kTileY - 1) / kTileY, B); }

}  // namespace

extern "C" int og_perspective_transform(int32_t batch, const float* src, const float* dst, double* M, void* stream) {
    og_clear_status();
    if (!src || !dst || !M) return OG_E_INVALID;
    if (batch < 1 || batch > 65535) return OG_E_SHAPE;
    if (((uintptr_t)src | (uintptr_t)dst) & 3 || (uintptr_t)M & 7) return OG_E_ALIGN;
    hipLaunchKernelGGL(perspective_transform_kernel, dim3((batch + kSolveThreads - 1) / kSolveThreads), dim3(kSolveThreads), 0, (hipStream_t)stream,
                       batch, src, dst, M);
    return og_launch_status();
}

extern "C" int og_warp_perspective_u8(int32_t batch, int32_t H, int32_t W, int32_t C, const uint8_t* src, const double* M, int32_t x0, int32_t y0,
                                      int32_t w, int32_t h, uint8_t* dst, void* stream) {
    og_clear_status();
    if (!src || !M || !dst) return OG_E_INVALID;
    if (!frame_ok(batch, H, W, C) || w < 1 || h < 1 || x0 < 0 || y0 < 0 || x0 > W - w || y0 > H - h) return OG_E_SHAPE;
    if ((uintptr_t)M & 7) return OG_E_ALIGN;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid = tiles(w, h, batch), block(kTileX, kTileY);
    if (C == 1) hipLaunchKernelGGL(warp_u8_kernel<1>, grid, block, 0, st, H, W, src, M, x0, y0, w, h, dst);
    else hipLaunchKernelGGL(warp_u8_kernel<3>, grid, block, 0, st, H, W, src, M, x0, y0, w, h, dst);
    return og_launch_status();
}

extern "C" int og_homography_pairs(int32_t batch, int32_t H, int32_t W, int32_t C, const uint8_t* frames, int32_t offset, const float* warp_offset,
                                   float* image0, float* image1, float* H_true, void* workspace_dev, void* stream) {
    og_clear_status();
    if (!frames || !image0 || !image1 || !workspace_dev || (warp_offset && !H_true)) return OG_E_INVALID;
    if (!frame_ok(batch, H, W, C) || offset < 0 || 2 * (int64_t)offset >= (H < W ? H : W)) return OG_E_SHAPE;
    if ((uintptr_t)workspace_dev & 7 || ((uintptr_t)image0 | (uintptr_t)image1 | (uintptr_t)H_true | (uintptr_t)warp_offset) & 3) return OG_E_ALIGN;
    hipStream_t st = (hipStream_t)stream;
    double* H_warp = (double*)workspace_dev;
    if (warp_offset)
        hipLaunchKernelGGL(pairs_solve_kernel, dim3((2 * batch + kSolveThreads - 1) / kSolveThreads), dim3(kSolveThreads), 0, st, batch, H, W, offset,
                           warp_offset, H_warp, H_true);
    const dim3 grid = tiles(W - 2 * offset, H - 2 * offset, batch), block(kTileX, kTileY);
    if (C == 1) hipLaunchKernelGGL(pairs_kernel<1>, grid, block, 0, st, H, W, frames, H_warp, offset, image0, image1);
    else hipLaunchKernelGGL(pairs_kernel<3>, grid, block, 0, st, H, W, frames, H_warp, offset, image0, image1);
    return og_launch_status();
}
