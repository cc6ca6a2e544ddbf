// SIFT keypoint extractor (DoG detector + SIFT / RootSIFT descriptor), a drop-in for the reference's OPENCV_SIFT feature path
// (models/features/opencv/{_features,base,torch_wrapper}.py), inference only.  Lowe 2004 with OpenCV's constants: 3 layers per
// octave, sigma 1.6, first octave -1, assumed input blur 0.5, contrast and edge tests off (the reference disables them and selects
// by radius NMS + top-k afterwards).  The float64 restatement is tests/sift_ref.py; DESIGN.md section 4.11 lists the known
// differences from OpenCV.
//
// Per-image buffers: gauss [octave][6][h][w] and dog [octave][5][h][w], fp32, octaves packed one after the other (SiftGeom).
// Stages (og_sift_pyramid / _detect / _orient / _describe / _select / _gather, include/openglue_amd.h):
//   pyramid   quantise to 8 bits + bilinear 2x upsample; every Gaussian level is one launch: a 64 x 64 tile and its halo in LDS, rows
//             then columns, fp32 accumulation, reflect-101 borders (any number of bounces); the DoG layer is written by the same launch.
//   detect    one thread per DoG sample: 26-neighbour extremum test, then the Newton refinement in fp64 (explicit cofactor solve, no
//             contraction, so the discrete decisions are those of the restatement).  Survivors are flagged, counted per 256-column
//             row segment, scanned, and written in (octave, layer, row, column) order of the extremum they started from: no atomics.
//   orient    one wave per keypoint: 36-bin histogram in fp64, accumulated in LDS as 2^-40 fixed point (integer atomics: the sum does
//             not depend on the order of the adds), smoothing, peaks >= 0.8 max by descending height; scan; one keypoint per peak.
//   describe  one workgroup per oriented keypoint: 4 x 4 x 8 trilinear histogram in LDS as 2^-38 fixed point, then normalise / clip /
//             renormalise / quantise / RootSIFT.
//   select    rank by (response desc, key asc, index asc) by counting; radius NMS equal to the greedy one: neighbour lists of
//             higher-ranked points (count, scan, fill), then rounds to the fixed point of "kept iff no kept higher-ranked neighbour";
//             top-k; min_stack over the batch.
//   gather    LAFs (lafs_from_opencv_kpts, mr_size 6), scores and descriptors of the kept keypoints in output order.
#include "og_block.h"
#include <cmath>

namespace {

constexpr int SIFT_S = 3, SIFT_LEVELS = SIFT_S + 3, SIFT_DOGS = SIFT_S + 2;
constexpr int SIFT_BORDER = 5, SIFT_MIN_SIDE = 2 * SIFT_BORDER + 1, SIFT_MAX_STEPS = 5;
constexpr int SIFT_MAX_OCT = 16;
constexpr int SIFT_RMAX = 13;                    // radius of the widest incremental blur (sigma 3.09)
constexpr int SIFT_TILE = 64;
constexpr int SIFT_SEG = 256;                    // columns per detection segment
constexpr int SIFT_MAX_PEAKS = 18;               // local maxima of a 36-bin circular histogram
constexpr int SIFT_NBR_AVG = 32;                 // neighbour-list capacity per oriented keypoint, on average
constexpr int SIFT_MIN_HW = 8, SIFT_MAX_HW = 8192;
constexpr int64_t SIFT_MAX_PIXELS = 1ll << 22;
constexpr double SIFT_SIGMA = 1.6;
constexpr double SIFT_ORI_FIX = 1099511627776.0;      // 2^40
constexpr double SIFT_DESC_FIX = 274877906944.0;      // 2^38

struct SiftGeom {
    int n;
    int h[SIFT_MAX_OCT], w[SIFT_MAX_OCT];
    int64_t goff[SIFT_MAX_OCT], doff[SIFT_MAX_OCT];  // float offsets of the octave in the per-image gauss / dog buffers
    int segbase[SIFT_MAX_OCT], nseg[SIFT_MAX_OCT];   // detection segments: ((l - 1) * (h - 10) + r - 5) * nseg + s
    int64_t gtot, dtot;
    int segtot;
    int cap, cap2;
    int64_t capn;
};

bool sift_shape_ok(int B, int H, int W) {
    return B > 0 && H >= SIFT_MIN_HW && W >= SIFT_MIN_HW && H <= SIFT_MAX_HW && W <= SIFT_MAX_HW && (int64_t)B * H * W <= SIFT_MAX_PIXELS;
}

SiftGeom sift_geom(int H, int W) {
    SiftGeom g{};
    int h = 2 * H, w = 2 * W;
    const int n = (int)std::floor(std::log2((double)(h < w ? h : w)) - 2.0 + 0.5) + 1;
    for (int o = 0; o < n && o < SIFT_MAX_OCT; ++o) {
        if (h < SIFT_MIN_SIDE || w < SIFT_MIN_SIDE) break;
        g.h[o] = h;
        g.w[o] = w;
        g.goff[o] = g.gtot;
        g.doff[o] = g.dtot;
        g.gtot += (int64_t)SIFT_LEVELS * h * w;
        g.dtot += (int64_t)SIFT_DOGS * h * w;
        g.nseg[o] = (w + SIFT_SEG - 1) / SIFT_SEG;
        g.segbase[o] = g.segtot;
        g.segtot += SIFT_S * (h - 2 * SIFT_BORDER) * g.nseg[o];
        g.n = o + 1;
        h /= 2;
        w /= 2;
    }
    const int64_t base = (int64_t)4 * H * W;
    g.cap = (int)(base / 8 > 1024 ? base / 8 : 1024);
    g.cap2 = g.cap + g.cap / 4;
    g.capn = (int64_t)SIFT_NBR_AVG * g.cap2;
    return g;
}

struct SiftTaps {
    int r;
    float t[2 * SIFT_RMAX + 1];
};

// radius (round(8 sigma + 1) | 1) / 2; exp(-x^2 / 2 sigma^2) normalised in fp64, stored as fp32
SiftTaps sift_taps(double sigma) {
    SiftTaps k{};
    k.r = ((int)std::floor(8.0 * sigma + 1.0 + 0.5) | 1) / 2;
    double t[2 * SIFT_RMAX + 1], sum = 0.0;
    for (int i = -k.r; i <= k.r; ++i) sum += t[i + k.r] = std::exp(-(double)(i * i) / (2.0 * sigma * sigma));
    for (int i = 0; i <= 2 * k.r; ++i) k.t[i] = (float)(t[i] / sum);
    return k;
}

double sift_level_sigma(int i) {
    if (i == 0) return std::sqrt(SIFT_SIGMA * SIFT_SIGMA - 1.0);
    const double a = SIFT_SIGMA * std::pow(2.0, (double)(i - 1) / SIFT_S), b = SIFT_SIGMA * std::pow(2.0, (double)i / SIFT_S);
    return std::sqrt(b * b - a * a);
}

__device__ __forceinline__ int reflect101(int i, int n) {
    const int p = 2 * (n - 1);
    i %= p;
    if (i < 0) i += p;
    return i >= n ? p - i : i;
}

// ---------------------------------------------------------------- pyramid
// u = clamp(trunc(255.f * x), 0, 255); output pixel j samples (j + 0.5) / 2 - 0.5, borders replicated.  Exact in fp32.
__global__ __launch_bounds__(256) void sift_upsample_kernel(const float* __restrict__ img, int H, int W, float* __restrict__ up) {
    const int X = blockIdx.x * 256 + threadIdx.x, Y = blockIdx.y, b = blockIdx.z;
    if (X >= 2 * W) return;
    const float* im = img + (int64_t)b * H * W;
    auto u = [&](int y, int x) { return fminf(fmaxf(truncf(255.f * im[(int64_t)y * W + x]), 0.f), 255.f); };
    const int my = Y >> 1, mx = X >> 1;
    const int y0 = (Y & 1) ? my : max(my - 1, 0), y1 = (Y & 1) ? min(my + 1, H - 1) : my;
    const int x0 = (X & 1) ? mx : max(mx - 1, 0), x1 = (X & 1) ? min(mx + 1, W - 1) : mx;
    const float wy0 = (Y & 1) ? 0.75f : 0.25f, wx0 = (X & 1) ? 0.75f : 0.25f;
    const float a = wy0 * u(y0, x0) + (1.f - wy0) * u(y1, x0), c = wy0 * u(y0, x1) + (1.f - wy0) * u(y1, x1);
    up[((int64_t)b * 2 * H + Y) * 2 * W + X] = wx0 * a + (1.f - wx0) * c;
}

// dst = Gaussian(src), one [h][w] plane per image (strides in floats); dog, when given, receives dst - src.
__global__ __launch_bounds__(256) void sift_blur_kernel(const float* __restrict__ src, int64_t src_stride, float* __restrict__ dst,
                                                        int64_t dst_stride, float* __restrict__ dog, int64_t dog_stride, int h, int w,
                                                        SiftTaps k) {
    constexpr int TW = SIFT_TILE + 2 * SIFT_RMAX;
    __shared__ float in[TW][TW + 1];
    __shared__ float mid[TW][SIFT_TILE + 1];
    const int R = k.r, tid = threadIdx.x;
    const int x0 = blockIdx.x * SIFT_TILE, y0 = blockIdx.y * SIFT_TILE;
    const float* s = src + (int64_t)blockIdx.z * src_stride;
    const int span = SIFT_TILE + 2 * R;
    for (int f = tid; f < span * span; f += 256) {
        const int rr = f / span, cc = f - rr * span;
        in[rr][cc] = s[(int64_t)reflect101(y0 - R + rr, h) * w + reflect101(x0 - R + cc, w)];
    }
    __syncthreads();
    for (int f = tid; f < span * SIFT_TILE; f += 256) {
        const int rr = f >> 6, cc = f & 63;
        float acc = 0.f;
        for (int t = 0; t <= 2 * R; ++t) acc = fmaf(k.t[t], in[rr][cc + t], acc);
        mid[rr][cc] = acc;
    }
    __syncthreads();
    for (int f = tid; f < SIFT_TILE * SIFT_TILE; f += 256) {
        const int rr = f >> 6, cc = f & 63;
        const int y = y0 + rr, x = x0 + cc;
        if (y >= h || x >= w) continue;
        float acc = 0.f;
        for (int t = 0; t <= 2 * R; ++t) acc = fmaf(k.t[t], mid[rr + t][cc], acc);
        dst[(int64_t)blockIdx.z * dst_stride + (int64_t)y * w + x] = acc;
        if (dog) dog[(int64_t)blockIdx.z * dog_stride + (int64_t)y * w + x] = acc - in[rr + R][cc + R];
    }
}

// every second pixel from 0 of the previous octave's image S
__global__ __launch_bounds__(256) void sift_decimate_kernel(const float* __restrict__ src, int64_t stride, int ws, float* __restrict__ dst,
                                                            int h, int w) {
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x >= w) return;
    dst[(int64_t)blockIdx.z * stride + (int64_t)y * w + x] = src[(int64_t)blockIdx.z * stride + (int64_t)(2 * y) * ws + 2 * x];
}

// ---------------------------------------------------------------- detect
struct SiftRefined {
    int l, r, c;
    double x, y, size, resp;
};

// Up to 5 Newton steps on the 3-D quadratic around DoG sample (l, r, c) of octave o (d: the octave's [5][h][w] block), in fp64
// with the operation order of tests/sift_ref.py refine(); no contraction, so both sides take the same discrete decisions.
__device__ bool sift_refine(const float* __restrict__ d, int h, int w, int o, int l, int r, int c, SiftRefined& out) {
#pragma clang fp contract(off)
    const int64_t ls = (int64_t)h * w;
    for (int it = 0; it < SIFT_MAX_STEPS; ++it) {
        const float* p = d + l * ls + (int64_t)r * w + c;
        auto at = [&](int dl, int dr, int dc) { return (double)p[dl * ls + (int64_t)dr * w + dc]; };
        const double v = at(0, 0, 0);
        const double gx = 0.5 * (at(0, 0, 1) - at(0, 0, -1));
        const double gy = 0.5 * (at(0, 1, 0) - at(0, -1, 0));
        const double gs = 0.5 * (at(1, 0, 0) - at(-1, 0, 0));
        const double v2 = 2.0 * v;
        const double dxx = at(0, 0, 1) + at(0, 0, -1) - v2;
        const double dyy = at(0, 1, 0) + at(0, -1, 0) - v2;
        const double dss = at(1, 0, 0) + at(-1, 0, 0) - v2;
        const double dxy = 0.25 * (at(0, 1, 1) - at(0, 1, -1) - at(0, -1, 1) + at(0, -1, -1));
        const double dxs = 0.25 * (at(1, 0, 1) - at(1, 0, -1) - at(-1, 0, 1) + at(-1, 0, -1));
        const double dys = 0.25 * (at(1, 1, 0) - at(1, -1, 0) - at(-1, 1, 0) + at(-1, -1, 0));
        const double c00 = dyy * dss - dys * dys;
        const double c01 = dxs * dys - dxy * dss;
        const double c02 = dxy * dys - dxs * dyy;
        const double c11 = dxx * dss - dxs * dxs;
        const double c12 = dxy * dxs - dxx * dys;
        const double c22 = dxx * dyy - dxy * dxy;
        const double det = dxx * c00 + dxy * c01 + dxs * c02;
        if (det == 0.0) return false;
        const double xc = -(c00 * gx + c01 * gy + c02 * gs) / det;
        const double xr = -(c01 * gx + c11 * gy + c12 * gs) / det;
        const double xl = -(c02 * gx + c12 * gy + c22 * gs) / det;
        if (fabs(xc) < 0.5 && fabs(xr) < 0.5 && fabs(xl) < 0.5) {
            const double scale = ldexp(1.0, o - 1);
            out.l = l;
            out.r = r;
            out.c = c;
            out.x = ((double)c + xc) * scale - 0.25;
            out.y = ((double)r + xr) * scale - 0.25;
            out.size = 2.0 * (SIFT_SIGMA * exp2(((double)l + xl) / 3.0) * scale);
            out.resp = fabs(v + 0.5 * (gx * xc + gy * xr + gs * xl)) / 255.0;
            return true;
        }
        if (!(fabs(xc) < 1e6) || !(fabs(xr) < 1e6) || !(fabs(xl) < 1e6)) return false;
        c += (int)floor(xc + 0.5);
        r += (int)floor(xr + 0.5);
        l += (int)floor(xl + 0.5);
        if (l < 1 || l > SIFT_S || c < SIFT_BORDER || c >= w - SIFT_BORDER || r < SIFT_BORDER || r >= h - SIFT_BORDER) return false;
    }
    return false;
}

// Workgroup (segment, layer * row, image) of one octave: flags the samples that are extrema and survive the refinement.
__global__ __launch_bounds__(256) void sift_extrema_kernel(const float* __restrict__ dog, int64_t dtot, int64_t doff, int h, int w, int o,
                                                           uint8_t* __restrict__ mask, int32_t* __restrict__ seg, int segtot, int segbase) {
    const int rows = h - 2 * SIFT_BORDER;
    const int s = blockIdx.x, row = blockIdx.y, b = blockIdx.z, tid = threadIdx.x;
    const int l = 1 + row / rows, r = SIFT_BORDER + row % rows, c = s * SIFT_SEG + tid;
    const float* d = dog + (int64_t)b * dtot + doff;
    const int64_t ls = (int64_t)h * w;
    int keep = 0;
    if (c >= SIFT_BORDER && c < w - SIFT_BORDER) {
        const float* p = d + l * ls + (int64_t)r * w + c;
        const float v = p[0];
        if (v != 0.f) {
            bool ok = true;
            for (int dl = -1; dl <= 1 && ok; ++dl)
                for (int dr = -1; dr <= 1; ++dr)
                    for (int dc = -1; dc <= 1; ++dc) {
                        const float nb = p[dl * ls + (int64_t)dr * w + dc];
                        ok = ok && (v > 0.f ? v >= nb : v <= nb);
                    }
            if (ok) {
                SiftRefined q;
                keep = sift_refine(d, h, w, o, l, r, c, q);
            }
        }
        mask[(int64_t)b * dtot + doff + l * ls + (int64_t)r * w + c] = (uint8_t)keep;
    }
    const int cnt = __syncthreads_count(keep);
    if (tid == 0) seg[(int64_t)b * segtot + segbase + row * gridDim.x + s] = cnt;
}

// exclusive scan of a[b * stride + 0 .. n) in place (n = n_fixed, or min(n_dev[b], ncap)), total -> total[b]; the body is og_block.h's
__global__ __launch_bounds__(256) void sift_scan_kernel(int32_t* __restrict__ a, int64_t stride, int n_fixed, const int32_t* __restrict__ n_dev,
                                                        int ncap, int32_t* __restrict__ total) {
    const int b = blockIdx.x;
    block_exclusive_scan_inplace(a + (int64_t)b * stride, n_dev ? min(n_dev[b], ncap) : n_fixed, total + b);
}

// the flagged samples of one segment, refined again and written at the segment's scanned offset in column order
__global__ __launch_bounds__(256) void sift_compact_kernel(const float* __restrict__ dog, int64_t dtot, int64_t doff, int h, int w, int o,
                                                           const uint8_t* __restrict__ mask, const int32_t* __restrict__ seg, int segtot,
                                                           int segbase, int cap, int32_t* __restrict__ det_i, double* __restrict__ det_f) {
    __shared__ int wsum[4];
    const int rows = h - 2 * SIFT_BORDER;
    const int s = blockIdx.x, row = blockIdx.y, b = blockIdx.z;
    const int l = 1 + row / rows, r = SIFT_BORDER + row % rows, c = s * SIFT_SEG + (int)threadIdx.x;
    const int64_t ls = (int64_t)h * w;
    const bool keep = c >= SIFT_BORDER && c < w - SIFT_BORDER && mask[(int64_t)b * dtot + doff + l * ls + (int64_t)r * w + c];
    int cnt;
    const int rank = block_rank_of(keep, wsum, cnt);
    if (!keep) return;
    const int off = seg[(int64_t)b * segtot + segbase + row * gridDim.x + s] + rank;
    if (off >= cap) return;                       // reported: counts[b] > capacity
    SiftRefined q;
    if (!sift_refine(dog + (int64_t)b * dtot + doff, h, w, o, l, r, c, q)) return;      // cannot happen: the flag says it converged
    int32_t* ki = det_i + ((int64_t)b * cap + off) * 4;
    double* kf = det_f + ((int64_t)b * cap + off) * 4;
    ki[0] = o; ki[1] = q.l; ki[2] = q.r; ki[3] = q.c;
    kf[0] = q.x; kf[1] = q.y; kf[2] = q.size; kf[3] = q.resp;
}

// ---------------------------------------------------------------- orient
// One wave per keypoint.  peaks[b][i][.]: angles in degrees by descending peak height; npeaks[b][i] their number.
__global__ __launch_bounds__(64) void sift_orient_kernel(const float* __restrict__ gauss, int64_t gtot, SiftGeom g, int upright,
                                                         const int32_t* __restrict__ det_i, const double* __restrict__ det_f,
                                                         const int32_t* __restrict__ counts, int32_t* __restrict__ npeaks,
                                                         float* __restrict__ peaks) {
    __shared__ unsigned long long hq[36];
    __shared__ double hr[36], hs[36];
    const int i = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    if (i >= min(counts[b], g.cap)) return;
    const int64_t rec = (int64_t)b * g.cap + i;
    if (upright) {
        if (tid == 0) {
            npeaks[rec] = 1;
            peaks[rec * SIFT_MAX_PEAKS] = 0.f;
        }
        return;
    }
    const int o = det_i[rec * 4], l = det_i[rec * 4 + 1], r = det_i[rec * 4 + 2], c = det_i[rec * 4 + 3];
    const int h = g.h[o], w = g.w[o];
    const float* img = gauss + (int64_t)b * gtot + g.goff[o] + (int64_t)l * h * w;
    const double sg = (double)(float)det_f[rec * 4 + 2] * 0.5 / ldexp(1.0, o - 1);       // from the float32 size a cv2.KeyPoint holds
    const int rad = (int)floor(4.5 * sg + 0.5);
    const double es = -1.0 / (2.0 * (1.5 * sg) * (1.5 * sg));
    if (tid < 36) hq[tid] = 0ull;
    __syncthreads();
    const int side = 2 * rad + 1;
    for (int f = tid; f < side * side; f += 64) {
        const int di = f / side - rad, dj = f % side - rad;
        const int y = r + di, x = c + dj;
        if (y <= 0 || y >= h - 1 || x <= 0 || x >= w - 1) continue;
        const double dx = (double)img[(int64_t)y * w + x + 1] - (double)img[(int64_t)y * w + x - 1];
        const double dy = (double)img[(int64_t)(y + 1) * w + x] - (double)img[(int64_t)(y - 1) * w + x];
        const double wgt = exp((double)(di * di + dj * dj) * es);
        const double mag = sqrt(dx * dx + dy * dy);
        int bin = (int)floor(atan2(dy, dx) * (180.0 / M_PI) * (36.0 / 360.0) + 0.5) % 36;
        if (bin < 0) bin += 36;
        atomicAdd(&hq[bin], (unsigned long long)__double2ll_rn(wgt * mag * SIFT_ORI_FIX));
    }
    __syncthreads();
    if (tid < 36) hr[tid] = (double)(long long)hq[tid] * (1.0 / SIFT_ORI_FIX);
    __syncthreads();
    if (tid < 36) {
        const int j = tid;
        hs[j] = (hr[(j + 34) % 36] + hr[(j + 2) % 36]) * (1.0 / 16) + (hr[(j + 35) % 36] + hr[(j + 1) % 36]) * (4.0 / 16) + hr[j] * (6.0 / 16);
    }
    __syncthreads();
    if (tid == 0) {
        double mx = hs[0];
        for (int j = 1; j < 36; ++j) mx = fmax(mx, hs[j]);
        double ph[SIFT_MAX_PEAKS];
        float pa[SIFT_MAX_PEAKS];
        int np = 0;
        for (int j = 0; j < 36; ++j) {
            const double lft = hs[(j + 35) % 36], rgt = hs[(j + 1) % 36], v = hs[j];
            if (!(v > lft && v > rgt && v >= 0.8 * mx)) continue;
            double bn = (double)j + 0.5 * (lft - rgt) / (lft - 2.0 * v + rgt);
            bn = bn < 0.0 ? bn + 36.0 : (bn >= 36.0 ? bn - 36.0 : bn);
            float ang = (float)(bn * 10.0);
            if (ang >= 360.f) ang = 0.f;
            int k = np++;                                   // insertion by descending height; equal heights keep bin order
            while (k > 0 && ph[k - 1] < v) {
                ph[k] = ph[k - 1];
                pa[k] = pa[k - 1];
                --k;
            }
            ph[k] = v;
            pa[k] = ang;
        }
        npeaks[rec] = np;
        for (int k = 0; k < np; ++k) peaks[rec * SIFT_MAX_PEAKS + k] = pa[k];
    }
}

// keypoint i -> its peaks at the scanned offset: ori_i = (octave, layer, row, column, orientation rank, source), ori_f = (x, y,
// size, angle, response) in float32, as a cv2.KeyPoint holds them
__global__ __launch_bounds__(256) void sift_expand_kernel(SiftGeom g, const int32_t* __restrict__ det_i, const double* __restrict__ det_f,
                                                          const int32_t* __restrict__ counts, const int32_t* __restrict__ offs,
                                                          const int32_t* __restrict__ counts_ori, const float* __restrict__ peaks,
                                                          int32_t* __restrict__ ori_i, float* __restrict__ ori_f) {
    const int i = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
    const int n = min(counts[b], g.cap);
    if (i >= n) return;
    const int64_t rec = (int64_t)b * g.cap + i;
    const int off = offs[rec];
    const int np = (i + 1 < n ? offs[rec + 1] : counts_ori[b]) - off;
    for (int k = 0; k < np; ++k) {
        if (off + k >= g.cap2) return;            // reported: counts[B + b] > capacity
        const int64_t out = (int64_t)b * g.cap2 + off + k;
        int32_t* oi = ori_i + out * 6;
        float* of = ori_f + out * 5;
        for (int e = 0; e < 4; ++e) oi[e] = det_i[rec * 4 + e];
        oi[4] = k;
        oi[5] = i;
        of[0] = (float)det_f[rec * 4];
        of[1] = (float)det_f[rec * 4 + 1];
        of[2] = (float)det_f[rec * 4 + 2];
        of[3] = peaks[rec * SIFT_MAX_PEAKS + k];
        of[4] = (float)det_f[rec * 4 + 3];
    }
}

// ---------------------------------------------------------------- describe
__device__ __forceinline__ float sift_block_sum128(float v, float* red) {      // threads 0..127 hold v; fixed order: deterministic
    const int tid = threadIdx.x;
    const float s = wave_sum(tid < 128 ? v : 0.f);
    __syncthreads();
    if ((tid & 63) == 0) red[tid >> 6] = s;
    __syncthreads();
    return red[0] + red[1];
}

__global__ __launch_bounds__(256) void sift_describe_kernel(const float* __restrict__ gauss, int64_t gtot, SiftGeom g, int quantize,
                                                            int rootsift, const int32_t* __restrict__ ori_i, const float* __restrict__ ori_f,
                                                            const int32_t* __restrict__ counts_ori, float* __restrict__ desc) {
    __shared__ unsigned long long hq[128];
    __shared__ float red[4];
    const int i = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    if (i >= min(counts_ori[b], g.cap2)) return;
    const int64_t rec = (int64_t)b * g.cap2 + i;
    const int o = ori_i[rec * 6], l = ori_i[rec * 6 + 1], r = ori_i[rec * 6 + 2], c = ori_i[rec * 6 + 3];
    const int h = g.h[o], w = g.w[o];
    const float* img = gauss + (int64_t)b * gtot + g.goff[o] + (int64_t)l * h * w;
    const double angle = (double)ori_f[rec * 5 + 3];
    const double hw = 3.0 * ((double)ori_f[rec * 5 + 2] * 0.5 / ldexp(1.0, o - 1));
    int rad = (int)floor(hw * 1.4142135623730951 * 2.5 + 0.5);
    rad = min(rad, (int)sqrt((double)h * h + (double)w * w));
    const double th = angle * (M_PI / 180.0);
    const float ct = (float)(cos(th) / hw), st = (float)(sin(th) / hw), ang0 = (float)angle;
    if (tid < 128) hq[tid] = 0ull;
    __syncthreads();
    const int side = 2 * rad + 1;
    for (int f = tid; f < side * side; f += 256) {
        const int di = f / side - rad, dj = f % side - rad;
        const float crot = (float)dj * ct + (float)di * st, rrot = (float)di * ct - (float)dj * st;
        const float rbin = rrot + 1.5f, cbin = crot + 1.5f;
        const int y = r + di, x = c + dj;
        if (!(rbin > -1.f && rbin < 4.f && cbin > -1.f && cbin < 4.f) || y <= 0 || y >= h - 1 || x <= 0 || x >= w - 1) continue;
        const float dx = img[(int64_t)y * w + x + 1] - img[(int64_t)y * w + x - 1];
        const float dy = img[(int64_t)(y + 1) * w + x] - img[(int64_t)(y - 1) * w + x];
        const float obin = (atan2f(dy, dx) * 57.29577951308232f - ang0) * (8.f / 360.f);
        const float mag = sqrtf(dx * dx + dy * dy) * expf((crot * crot + rrot * rrot) * (-1.f / 8.f));
        const float r0f = floorf(rbin), c0f = floorf(cbin), o0f = floorf(obin);
        // obin is a product; contracted with this subtraction it is not rounded first, and where it rounds up to an integer (a
        // gradient exactly along the keypoint's axes) the fraction comes out as -1e-7, a negative weight and, under the RootSIFT
        // square root of the float path, a NaN.  The weights are clamped to what they mean.
        const float fr = rbin - r0f, fc = cbin - c0f, fo = fmaxf(obin - o0f, 0.f);
        const int r0 = (int)r0f, c0 = (int)c0f, o0 = (int)o0f;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int dr = e >> 2, dc = (e >> 1) & 1, dd = e & 1;
            const int rr = r0 + dr, cc = c0 + dc;
            if (rr < 0 || rr >= 4 || cc < 0 || cc >= 4) continue;
            const int oo = (o0 + dd) & 7;
            const float v = mag * (dr ? fr : 1.f - fr) * (dc ? fc : 1.f - fc) * (dd ? fo : 1.f - fo);
            atomicAdd(&hq[(rr * 4 + cc) * 8 + oo], (unsigned long long)__double2ll_rn((double)v * SIFT_DESC_FIX));
        }
    }
    __syncthreads();
    float v = tid < 128 ? (float)((double)(long long)hq[tid] * (1.0 / SIFT_DESC_FIX)) : 0.f;
    const float n1 = sqrtf(sift_block_sum128(v * v, red));
    if (n1 == 0.f) {                               // an all-zero histogram stays zero
        if (tid < 128) desc[rec * 128 + tid] = 0.f;
        return;
    }
    v = fminf(v / n1, 0.2f);
    const float n2 = sqrtf(sift_block_sum128(v * v, red));
    v = v / n2;
    if (quantize) v = fminf(255.f, floorf(512.f * v + 0.5f));
    if (rootsift > 0) {
        const float l1 = sift_block_sum128(v, red);
        v = l1 > 0.f ? sqrtf(v / l1) : 0.f;
    } else if (rootsift == 0) {
        const float l2 = sqrtf(sift_block_sum128(v * v, red));
        v = l2 > 0.f ? v / l2 : 0.f;
    }
    if (tid < 128) desc[rec * 128 + tid] = v;
}

// ---------------------------------------------------------------- select
__device__ __forceinline__ int64_t sift_key(const int32_t* oi) {
    return ((((int64_t)oi[0] * 4 + oi[1]) * 65536 + oi[2]) * 65536 + oi[3]) * 32 + oi[4];
}

// order[rank] = index, rank = number of keypoints that come first under (response desc, key asc, index asc)
__global__ __launch_bounds__(256) void sift_rank_kernel(int cap2, const int32_t* __restrict__ ori_i, const float* __restrict__ ori_f,
                                                        const int32_t* __restrict__ counts_ori, int32_t* __restrict__ order) {
    __shared__ float sr[256];
    __shared__ int64_t sk[256];
    const int b = blockIdx.y, tid = threadIdx.x;
    const int n = min(counts_ori[b], cap2);
    if (blockIdx.x * 256 >= n) return;
    const int i = blockIdx.x * 256 + tid;
    const bool live = i < n;
    const int64_t base = (int64_t)b * cap2;
    const float v = live ? ori_f[(base + i) * 5 + 4] : 0.f;
    const int64_t key = live ? sift_key(ori_i + (base + i) * 6) : 0;
    int rank = 0;
    for (int j0 = 0; j0 < n; j0 += 256) {
        __syncthreads();
        if (j0 + tid < n) {
            sr[tid] = ori_f[(base + j0 + tid) * 5 + 4];
            sk[tid] = sift_key(ori_i + (base + j0 + tid) * 6);
        }
        __syncthreads();
        const int lim = min(256, n - j0);
        for (int j = 0; j < lim; ++j) {
            const float u = sr[j];
            rank += (u > v) || (u == v && (sk[j] < key || (sk[j] == key && j0 + j < i)));
        }
    }
    if (live) order[base + rank] = i;
}

// Neighbours of rank p among the ranks q < p: distance <= radius on the float32 positions, in fp64 (the reference's KDTree query).
// FILL = false: nbr_cnt[p] = their number; FILL = true: the ranks q, ascending, at nbr[nbr_off[p] ..).
template <bool FILL>
__global__ __launch_bounds__(256) void sift_neighbours_kernel(int cap2, int64_t capn, double r2, const float* __restrict__ ori_f,
                                                              const int32_t* __restrict__ counts_ori, const int32_t* __restrict__ order,
                                                              int32_t* __restrict__ nbr_cnt, int32_t* __restrict__ nbr) {
    __shared__ float sx[256], sy[256];
    const int b = blockIdx.y, tid = threadIdx.x;
    const int n = min(counts_ori[b], cap2);
    if (blockIdx.x * 256 >= n) return;
    const int p = blockIdx.x * 256 + tid;
    const bool live = p < n;
    const int64_t base = (int64_t)b * cap2;
    double x = 0.0, y = 0.0;
    if (live) {
        const int i = order[base + p];
        x = (double)ori_f[(base + i) * 5];
        y = (double)ori_f[(base + i) * 5 + 1];
    }
    int cnt = 0;
    const int64_t out = FILL && live ? (int64_t)nbr_cnt[base + p] : 0;      // after the scan: the exclusive offset
    for (int q0 = 0; q0 <= (int)blockIdx.x * 256; q0 += 256) {
        __syncthreads();
        if (q0 + tid < n) {
            const int j = order[base + q0 + tid];
            sx[tid] = ori_f[(base + j) * 5];
            sy[tid] = ori_f[(base + j) * 5 + 1];
        }
        __syncthreads();
        const int lim = live ? min(256, p - q0) : 0;
        for (int q = 0; q < lim; ++q) {
            const double dx = (double)sx[q] - x, dy = (double)sy[q] - y;
            if (dx * dx + dy * dy <= r2) {
                if (FILL && out >= 0 && out + cnt < capn) nbr[(int64_t)b * capn + out + cnt] = q0 + q;
                ++cnt;
            }
        }
    }
    if (!FILL && live) nbr_cnt[base + p] = cnt;
}

// Rounds to the fixed point of "kept iff no kept neighbour of higher rank", one workgroup per image.  state[p]: 0 undecided, 1 kept,
// 2 suppressed.  A point is decided once all its higher-ranked neighbours are; the highest-ranked undecided point always is, so
// every sweep decides at least one and the loop ends.  Decisions do not depend on when a neighbour's state is seen.
__global__ __launch_bounds__(1024) void sift_nms_kernel(int cap2, int64_t capn, int nms, const int32_t* __restrict__ counts_ori,
                                                        const int32_t* __restrict__ nbr_off, const int32_t* __restrict__ nbr_total,
                                                        const int32_t* __restrict__ nbr, int32_t* __restrict__ state) {
    const int b = blockIdx.x, tid = threadIdx.x;
    const int n = min(counts_ori[b], cap2);
    int32_t* st = state + (int64_t)b * cap2;
    for (int p = tid; p < n; p += 1024) st[p] = nms ? 0 : 1;
    if (!nms) return;
    const int32_t* off = nbr_off + (int64_t)b * cap2;
    const int32_t* nb = nbr + (int64_t)b * capn;
    const int64_t tot = nbr_total[b];
    if (tot < 0 || tot > capn) return;            // reported: counts[3B + b] out of capacity; nothing is kept
    __syncthreads();
    for (int sweep = 0; sweep <= n; ++sweep) {
        int changed = 0;
        for (int p = tid; p < n; p += 1024) {
            if (__hip_atomic_load(&st[p], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0) continue;
            const int64_t lo = off[p], hi = p + 1 < n ? off[p + 1] : tot;
            bool any_kept = false, all_decided = true;
            for (int64_t e = lo; e < hi; ++e) {
                const int s = __hip_atomic_load(&st[nb[e]], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                any_kept = any_kept || s == 1;
                all_decided = all_decided && s != 0;
            }
            if (any_kept || all_decided) {
                __hip_atomic_store(&st[p], any_kept ? 2 : 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                changed = 1;
            }
        }
        if (!__syncthreads_or(changed)) break;
    }
}

// kept ranks -> sel[b][position] = keypoint index, in rank order; counts[2B + b] = min(kept, max_kpts)
__global__ __launch_bounds__(256) void sift_keep_kernel(int B, int cap2, int max_kpts, const int32_t* __restrict__ counts_ori,
                                                        const int32_t* __restrict__ order, const int32_t* __restrict__ state,
                                                        int32_t* __restrict__ sel, int32_t* __restrict__ counts) {
    __shared__ int32_t part[256];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int n = min(counts_ori[b], cap2);
    const int64_t base = (int64_t)b * cap2;
    const int per = (n + 255) / 256;
    const int lo = min(tid * per, n), hi = min(lo + per, n);
    int sum = 0;
    for (int p = lo; p < hi; ++p) sum += state[base + p] == 1;
    part[tid] = sum;
    __syncthreads();
    if (tid == 0) {
        int run = 0;
        for (int i = 0; i < 256; ++i) {
            const int v = part[i];
            part[i] = run;
            run += v;
        }
        counts[2 * B + b] = max_kpts > 0 && max_kpts < run ? max_kpts : run;
    }
    __syncthreads();
    int run = part[tid];
    for (int p = lo; p < hi; ++p)
        if (state[base + p] == 1) sel[base + run++] = order[base + p];
}

// min_stack: every image is cut to the batch-minimum count
__global__ void sift_min_kernel(int B, int32_t* __restrict__ counts) {
    int m = counts[2 * B];
    for (int b = 1; b < B; ++b) m = min(m, counts[2 * B + b]);
    counts[4 * B] = m;
}

// lafs_from_opencv_kpts (mr_size 6): scale 6 size, angle deg2rad(-angle); scores; descriptors.  128 threads per keypoint.
__global__ __launch_bounds__(128) void sift_gather_kernel(int cap2, int n, const int32_t* __restrict__ sel, const float* __restrict__ ori_f,
                                                          const float* __restrict__ desc, float* __restrict__ lafs, float* __restrict__ scores,
                                                          float* __restrict__ out) {
    const int k = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const int64_t src = (int64_t)b * cap2 + sel[(int64_t)b * cap2 + k];
    const int64_t dst = (int64_t)b * n + k;
    if (tid == 0) {
        const float* of = ori_f + src * 5;
        const float s = 6.f * of[2], a = -of[3] * 0.017453292519943295f;
        const float sc = s * cosf(a), ss = s * sinf(a);
        float* L = lafs + dst * 6;
        L[0] = sc; L[1] = ss; L[2] = of[0];
        L[3] = -ss; L[4] = sc; L[5] = of[1];
        scores[dst] = of[4];
    }
    out[dst * 128 + tid] = desc[src * 128 + tid];
}

// ---------------------------------------------------------------- workspace
struct SiftWs {
    float* up;               // [B][2H][2W] upsampled base image (pyramid)
    uint8_t* mask;           // [B][dtot] (detect)
    int32_t* seg;            // [B][segtot]
    int32_t* npeaks;         // [B][cap] (orient): counts, then offsets
    float* peaks;            // [B][cap][18]
    int32_t* order;          // [B][cap2] (select)
    int32_t* nbr_off;        // [B][cap2]
    int32_t* state;          // [B][cap2]
    int32_t* nbr;            // [B][capn]
    size_t bytes;
};
SiftWs sift_ws(void* base, int B, int H, int W, const SiftGeom& g) {
    char* p = (char*)base;
    size_t o = 0;
    SiftWs w{};
    auto take = [&](int64_t n) { char* q = p + o; o += og_round_up(n, 256); return q; };
    w.up = (float*)take((int64_t)B * 4 * H * W * 4);
    w.mask = (uint8_t*)take((int64_t)B * g.dtot);
    w.seg = (int32_t*)take((int64_t)B * g.segtot * 4);
    w.npeaks = (int32_t*)take((int64_t)B * g.cap * 4);
    w.peaks = (float*)take((int64_t)B * g.cap * SIFT_MAX_PEAKS * 4);
    w.order = (int32_t*)take((int64_t)B * g.cap2 * 4);
    w.nbr_off = (int32_t*)take((int64_t)B * g.cap2 * 4);
    w.state = (int32_t*)take((int64_t)B * g.cap2 * 4);
    w.nbr = (int32_t*)take((int64_t)B * g.capn * 4);
    w.bytes = o;
    return w;
}

}  // namespace

// out[0] = octaves, out[1] = keypoint capacity, out[2] = oriented-keypoint capacity, out[3 + 2 o], out[4 + 2 o] = h, w of octave o
extern "C" int og_sift_geometry(int32_t H, int32_t W, int32_t* out) {
    if (!out) return OG_E_INVALID;
    if (!sift_shape_ok(1, H, W)) return OG_E_INVALID;
    const SiftGeom g = sift_geom(H, W);
    out[0] = g.n;
    out[1] = g.cap;
    out[2] = g.cap2;
    for (int o = 0; o < SIFT_MAX_OCT; ++o) {
        out[3 + 2 * o] = o < g.n ? g.h[o] : 0;
        out[4 + 2 * o] = o < g.n ? g.w[o] : 0;
    }
    return 0;
}

extern "C" size_t og_sift_workspace_bytes(int32_t batch, int32_t H, int32_t W) {
    if (!sift_shape_ok(batch, H, W)) return 0;
    return sift_ws(nullptr, batch, H, W, sift_geom(H, W)).bytes;
}

extern "C" int og_sift_pyramid(int32_t batch, int32_t H, int32_t W, const float* image, float* gauss, float* dog, void* workspace_dev,
                               void* stream) {
    og_clear_status();
    if (!image || !gauss || !dog || !workspace_dev || !sift_shape_ok(batch, H, W)) return OG_E_INVALID;
    if ((uintptr_t)workspace_dev % 16) return OG_E_ALIGN;
    const SiftGeom g = sift_geom(H, W);
    const SiftWs ws = sift_ws(workspace_dev, batch, H, W, g);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(sift_upsample_kernel, dim3((2 * W + 255) / 256, 2 * H, batch), dim3(256), 0, st, image, H, W, ws.up);
    for (int o = 0; o < g.n; ++o) {
        const int h = g.h[o], w = g.w[o];
        const int64_t hw = (int64_t)h * w;
        const dim3 grid((w + SIFT_TILE - 1) / SIFT_TILE, (h + SIFT_TILE - 1) / SIFT_TILE, batch);
        float* go = gauss + g.goff[o];
        if (o == 0)
            hipLaunchKernelGGL(sift_blur_kernel, grid, dim3(256), 0, st, ws.up, hw, go, g.gtot, (float*)nullptr, (int64_t)0, h, w,
                               sift_taps(sift_level_sigma(0)));
        else
            hipLaunchKernelGGL(sift_decimate_kernel, dim3((w + 255) / 256, h, batch), dim3(256), 0, st,
                               gauss + g.goff[o - 1] + (int64_t)SIFT_S * g.h[o - 1] * g.w[o - 1], g.gtot, g.w[o - 1], go, h, w);
        for (int i = 1; i < SIFT_LEVELS; ++i)
            hipLaunchKernelGGL(sift_blur_kernel, grid, dim3(256), 0, st, go + (i - 1) * hw, g.gtot, go + i * hw, g.gtot,
                               dog + g.doff[o] + (i - 1) * hw, g.dtot, h, w, sift_taps(sift_level_sigma(i)));
    }
    return og_launch_status();
}

extern "C" int og_sift_detect(int32_t batch, int32_t H, int32_t W, const float* dog, int32_t* det_i, double* det_f, int32_t* counts,
                              void* workspace_dev, void* stream) {
    og_clear_status();
    if (!dog || !det_i || !det_f || !counts || !workspace_dev || !sift_shape_ok(batch, H, W)) return OG_E_INVALID;
    if ((uintptr_t)workspace_dev % 16) return OG_E_ALIGN;
    const SiftGeom g = sift_geom(H, W);
    const SiftWs ws = sift_ws(workspace_dev, batch, H, W, g);
    hipStream_t st = (hipStream_t)stream;
    for (int o = 0; o < g.n; ++o)
        hipLaunchKernelGGL(sift_extrema_kernel, dim3(g.nseg[o], SIFT_S * (g.h[o] - 2 * SIFT_BORDER), batch), dim3(256), 0, st, dog, g.dtot,
                           g.doff[o], g.h[o], g.w[o], o, ws.mask, ws.seg, g.segtot, g.segbase[o]);
    hipLaunchKernelGGL(sift_scan_kernel, dim3(batch), dim3(256), 0, st, ws.seg, (int64_t)g.segtot, g.segtot, (const int32_t*)nullptr, 0, counts);
    for (int o = 0; o < g.n; ++o)
        hipLaunchKernelGGL(sift_compact_kernel, dim3(g.nseg[o], SIFT_S * (g.h[o] - 2 * SIFT_BORDER), batch), dim3(256), 0, st, dog, g.dtot,
                           g.doff[o], g.h[o], g.w[o], o, ws.mask, ws.seg, g.segtot, g.segbase[o], g.cap, det_i, det_f);
    return og_launch_status();
}

extern "C" int og_sift_orient(int32_t batch, int32_t H, int32_t W, int32_t upright, const float* gauss, const int32_t* det_i,
                              const double* det_f, int32_t* counts, int32_t* ori_i, float* ori_f, void* workspace_dev, void* stream) {
    og_clear_status();
    if (!gauss || !det_i || !det_f || !counts || !ori_i || !ori_f || !workspace_dev || !sift_shape_ok(batch, H, W)) return OG_E_INVALID;
    if ((uintptr_t)workspace_dev % 16) return OG_E_ALIGN;
    const SiftGeom g = sift_geom(H, W);
    const SiftWs ws = sift_ws(workspace_dev, batch, H, W, g);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(sift_orient_kernel, dim3(g.cap, batch), dim3(64), 0, st, gauss, g.gtot, g, upright != 0, det_i, det_f, counts, ws.npeaks,
                       ws.peaks);
    hipLaunchKernelGGL(sift_scan_kernel, dim3(batch), dim3(256), 0, st, ws.npeaks, (int64_t)g.cap, 0, counts, g.cap, counts + batch);
    hipLaunchKernelGGL(sift_expand_kernel, dim3((g.cap + 255) / 256, batch), dim3(256), 0, st, g, det_i, det_f, counts, ws.npeaks, counts + batch,
                       ws.peaks, ori_i, ori_f);
    return og_launch_status();
}

extern "C" int og_sift_describe(int32_t batch, int32_t H, int32_t W, int32_t quantize, int32_t rootsift, const float* gauss,
                                const int32_t* ori_i, const float* ori_f, const int32_t* counts, float* desc, void* stream) {
    og_clear_status();
    if (!gauss || !ori_i || !ori_f || !counts || !desc || !sift_shape_ok(batch, H, W)) return OG_E_INVALID;
    const SiftGeom g = sift_geom(H, W);
    hipLaunchKernelGGL(sift_describe_kernel, dim3(g.cap2, batch), dim3(256), 0, (hipStream_t)stream, gauss, g.gtot, g, quantize != 0,
                       rootsift, ori_i, ori_f, counts + batch, desc);
    return og_launch_status();
}

extern "C" int og_sift_select(int32_t batch, int32_t H, int32_t W, float nms_diameter, int32_t max_kpts, const int32_t* ori_i,
                              const float* ori_f, int32_t* counts, int32_t* sel, void* workspace_dev, void* stream) {
    og_clear_status();
    if (!ori_i || !ori_f || !counts || !sel || !workspace_dev || !sift_shape_ok(batch, H, W) || !(nms_diameter == nms_diameter))
        return OG_E_INVALID;
    if ((uintptr_t)workspace_dev % 16) return OG_E_ALIGN;
    const SiftGeom g = sift_geom(H, W);
    const SiftWs ws = sift_ws(workspace_dev, batch, H, W, g);
    hipStream_t st = (hipStream_t)stream;
    const int32_t* cori = counts + batch;
    const dim3 grid((g.cap2 + 255) / 256, batch);
    const int nms = nms_diameter > 0.f;
    const double radius = (double)nms_diameter / 2.0;
    hipLaunchKernelGGL(sift_rank_kernel, grid, dim3(256), 0, st, g.cap2, ori_i, ori_f, cori, ws.order);
    if (nms) {
        hipLaunchKernelGGL(sift_neighbours_kernel<false>, grid, dim3(256), 0, st, g.cap2, g.capn, radius * radius, ori_f, cori, ws.order,
                           ws.nbr_off, ws.nbr);
        hipLaunchKernelGGL(sift_scan_kernel, dim3(batch), dim3(256), 0, st, ws.nbr_off, (int64_t)g.cap2, 0, cori, g.cap2, counts + 3 * batch);
        hipLaunchKernelGGL(sift_neighbours_kernel<true>, grid, dim3(256), 0, st, g.cap2, g.capn, radius * radius, ori_f, cori, ws.order,
                           ws.nbr_off, ws.nbr);
    } else {
        (void)hipMemsetAsync(counts + 3 * batch, 0, (size_t)batch * 4, st);
    }
    hipLaunchKernelGGL(sift_nms_kernel, dim3(batch), dim3(1024), 0, st, g.cap2, g.capn, nms, cori, ws.nbr_off, counts + 3 * batch, ws.nbr, ws.state);
    hipLaunchKernelGGL(sift_keep_kernel, dim3(batch), dim3(256), 0, st, batch, g.cap2, max_kpts, cori, ws.order, ws.state, sel, counts);
    hipLaunchKernelGGL(sift_min_kernel, dim3(1), dim3(1), 0, st, batch, counts);
    return og_launch_status();
}

extern "C" int og_sift_gather(int32_t batch, int32_t H, int32_t W, int32_t n, const int32_t* sel, const float* ori_f, const float* desc,
                              float* lafs, float* scores, float* descriptors, void* stream) {
    og_clear_status();
    if (!sift_shape_ok(batch, H, W) || n < 0) return OG_E_INVALID;
    const SiftGeom g = sift_geom(H, W);
    if (n > g.cap2) return OG_E_INVALID;
    if (n == 0) return 0;
    if (!sel || !ori_f || !desc || !lafs || !scores || !descriptors) return OG_E_INVALID;
    hipLaunchKernelGGL(sift_gather_kernel, dim3(n, batch), dim3(128), 0, (hipStream_t)stream, g.cap2, n, sel, ori_f, desc, lafs, scores,
                       descriptors);
    return og_launch_status();
}
