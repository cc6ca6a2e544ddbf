// SuperPointNetBn fine-tuning: train-mode BatchNorm2d between the convolutions of the extractor, forward and backward, exact fp32 on
// v_mfma_f32_32x32x2_f32, no atomics: every sum has a fixed order.  (reference models/features/superpoint/model.py:180-199 with the
// modules in train(); models/matching_module.py:29-31,77-81 `finetune: True`.)
//
// BatchNorm layers L = 0..8: bn1a, then the BatchNorm behind the 3x3 MFMA layer j = L - 1 of og_superpoint_dense.h (bn1b, 2a, 2b, 3a, 3b,
// 4a, 4b, and bnPa | bnDa as one layer of 512 channels).  bnPb / bnDb act at coarse resolution on token rows and are composed in Python
// from og_batchnorm_train_* (openglue_amd/superpoint.py).
//
//   forward      every convolution stores its RAW output z = conv(x) + b, and its epilogue leaves per-tile, per-channel
//                (pivot, sum (z - pivot), sum (z - pivot)^2) over the tile's valid pixels, pivot = the tile's first z.
//                sp_bn_stats_finish_kernel turns each tile's triple into (count, mean, M2) in float64, merges them pairwise in a fixed
//                order, writes mean, rstd, scale = gamma rstd, beta and updates the running statistics.  No pass normalises a
//                full-resolution map: the NEXT layer's loader applies sp_bn_act = relu(fmaf(z - mean, scale, beta)) to what it loads,
//                over the four window pixels and then the max behind a pooled layer (gamma may be negative: the pool cannot be taken
//                on z).  Saved: z of every layer (unpooled) and the coefficients.
//   reduce       dbeta = sum gy, dgamma = rstd sum gy (z - mean) with gy = the incoming gradient after the pool routing (first
//                maximum of the window in raster order, as sp_grad_at) and the mask y > 0, both decided by sp_bn_act -- the function the
//                forward used.  Per-tile fp32 partials (128 pixels), combined in tile order in float64.
//   dz           formed on load (sp_bn_dz) for the weight and data gradients: dz = scale (gy - dbeta / N - xhat dgamma / N), dense at
//                full resolution also where the pool routed gy to one pixel in four.
//   wgrad/dgrad  the kernels and the layer loop of og_superpoint_train.h, which SuperPointNet runs too, instantiated with these loaders
//                (the policy SpBn); the layer's input x is sp_bn_act of the layer below.
//                The convolution biases get no gradient here: the mean subtraction removes them (the caller returns exact zeros).
#include "og_superpoint_train.h"

namespace {

constexpr int SPB_LAYERS = SP_LAYERS + 1;                                   // BatchNorm layers, bn1a first
constexpr int kBnC[SPB_LAYERS] = {64, 64, 64, 64, 128, 128, 128, 128, 512};
constexpr int SPB_CHANNELS = 1280;                                          // sum of kBnC
constexpr int SPB_TILE = 128;                                               // pixels per flat tile (conv1a statistics, backward reductions)
int bn_offset(int L) {
    int o = 0;
    for (int i = 0; i < L; ++i) o += kBnC[i];
    return o;
}

// ---------------------------------------------------------------- the one activation function
// Forward value, ReLU mask and pool argmax all come from here.  The fmaf is explicit: a contraction the compiler chose differently in
// two kernels would flip a mask or an argmax.
// The mean is subtracted first: a fused shift = beta - mean scale cancels against z scale where |mean| >> sigma (two coarse pixels).
__device__ __forceinline__ float sp_bn_act(float z, float mu, float sc, float be) { return fmaxf(__builtin_fmaf(z - mu, sc, be), 0.f); }

// dz of one element: scale (gy - k1 - (z - mean) k2), k1 = dbeta / N, k2 = rstd dgamma / N
__device__ __forceinline__ float sp_bn_dz1(float gy, float z, float sc, float mu, float k1, float k2) {
    return sc * __builtin_fmaf(mu - z, k2, gy - k1);
}

// Per-channel coefficients of one BatchNorm layer.  Forward (saved): mean | rstd | scale = gamma rstd | beta, C floats each.
// Backward: k1 | k2.
struct SpBnCoef {
    const float *mu, *sc, *be, *k1, *k2;
};
SpBnCoef bn_coef(const float* fwd, const float* bwd, int C) { return {fwd, fwd + 2 * C, fwd + 3 * C, bwd, bwd ? bwd + C : nullptr}; }

// The layer's input activation at pixel (y, x) of the H x W map it convolves, channels c .. c + 3, from the raw output z of the layer
// below.  INPOOL: z is [B][Hz][Wz][C] with H = Hz / 2, W = Wz / 2 and the activation is the max over the window's four activations.
template <bool INPOOL>
__device__ __forceinline__ f32x4 sp_bn_act_at(const float* __restrict__ z, const float* __restrict__ cf, int b, int Hz, int Wz, int C, int y,
                                              int x, int c) {
    const f32x4 u = *reinterpret_cast<const f32x4*>(cf + c), s = *reinterpret_cast<const f32x4*>(cf + 2 * C + c);
    const f32x4 t = *reinterpret_cast<const f32x4*>(cf + 3 * C + c);
    f32x4 out;
    if constexpr (!INPOOL) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(z + (((int64_t)b * Hz + y) * Wz + x) * C + c);
#pragma unroll
        for (int e = 0; e < 4; ++e) out[e] = sp_bn_act(v[e], u[e], s[e], t[e]);
    } else {
        const float* z0 = z + (((int64_t)b * Hz + 2 * y) * Wz + 2 * x) * C + c;         // rows 2 y, 2 y + 1 < Hz; columns 2 x, 2 x + 1 < Wz
        const f32x4 v00 = *reinterpret_cast<const f32x4*>(z0), v01 = *reinterpret_cast<const f32x4*>(z0 + C);
        const f32x4 v10 = *reinterpret_cast<const f32x4*>(z0 + (int64_t)Wz * C), v11 = *reinterpret_cast<const f32x4*>(z0 + (int64_t)Wz * C + C);
#pragma unroll
        for (int e = 0; e < 4; ++e)
            out[e] = fmaxf(fmaxf(sp_bn_act(v00[e], u[e], s[e], t[e]), sp_bn_act(v01[e], u[e], s[e], t[e])),
                           fmaxf(sp_bn_act(v10[e], u[e], s[e], t[e]), sp_bn_act(v11[e], u[e], s[e], t[e])));
    }
    return out;
}

// gy and z at pixel (y, x) of a layer's H x W output map (before the pool), channels c .. c + 3.  !POOLED: g is [B][H][W][C], the gradient
// of the activation.  POOLED: g is [B][H/2][W/2][C], the gradient of the pooled activation; the pixel receives it iff it is the first of
// its window, in raster order, that holds the window's maximum activation, and that maximum is > 0.  A pixel outside every window gets 0.
template <bool POOLED>
__device__ __forceinline__ void sp_bn_gy(const float* __restrict__ g, const float* __restrict__ z, const SpBnCoef& k, int b, int H, int W,
                                         int C, int y, int x, int c, f32x4& gy, f32x4& zv) {
    const f32x4 u = *reinterpret_cast<const f32x4*>(k.mu + c), s = *reinterpret_cast<const f32x4*>(k.sc + c);
    const f32x4 t = *reinterpret_cast<const f32x4*>(k.be + c);
    if constexpr (!POOLED) {
        const int64_t o = (((int64_t)b * H + y) * W + x) * C + c;
        zv = *reinterpret_cast<const f32x4*>(z + o);
        const f32x4 gv = *reinterpret_cast<const f32x4*>(g + o);
#pragma unroll
        for (int e = 0; e < 4; ++e) gy[e] = sp_bn_act(zv[e], u[e], s[e], t[e]) > 0.f ? gv[e] : 0.f;
    } else {
        const int Hp = H / 2, Wp = W / 2, py = y >> 1, px = x >> 1;
        gy = f32x4{0.f, 0.f, 0.f, 0.f};
        if (py >= Hp || px >= Wp) {
            zv = *reinterpret_cast<const f32x4*>(z + (((int64_t)b * H + y) * W + x) * C + c);
            return;
        }
        const float* z0 = z + (((int64_t)b * H + 2 * py) * W + 2 * px) * C + c;
        f32x4 v[4];
        v[0] = *reinterpret_cast<const f32x4*>(z0);
        v[1] = *reinterpret_cast<const f32x4*>(z0 + C);
        v[2] = *reinterpret_cast<const f32x4*>(z0 + (int64_t)W * C);
        v[3] = *reinterpret_cast<const f32x4*>(z0 + (int64_t)W * C + C);
        const f32x4 gv = *reinterpret_cast<const f32x4*>(g + (((int64_t)b * Hp + py) * Wp + px) * C + c);
        const int me = (y & 1) * 2 + (x & 1);
        zv = me == 0 ? v[0] : me == 1 ? v[1] : me == 2 ? v[2] : v[3];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float a0 = sp_bn_act(v[0][e], u[e], s[e], t[e]), a1 = sp_bn_act(v[1][e], u[e], s[e], t[e]);
            const float a2 = sp_bn_act(v[2][e], u[e], s[e], t[e]), a3 = sp_bn_act(v[3][e], u[e], s[e], t[e]);
            const float m = fmaxf(fmaxf(a0, a1), fmaxf(a2, a3));
            const int win = a0 == m ? 0 : a1 == m ? 1 : a2 == m ? 2 : 3;
            gy[e] = (win == me && m > 0.f) ? gv[e] : 0.f;
        }
    }
}

template <bool POOLED>
__device__ __forceinline__ f32x4 sp_bn_dz(const float* __restrict__ g, const float* __restrict__ z, const SpBnCoef& k, int b, int H, int W,
                                          int C, int y, int x, int c) {
    f32x4 gy, zv, out;
    sp_bn_gy<POOLED>(g, z, k, b, H, W, C, y, x, c, gy, zv);
    const f32x4 s = *reinterpret_cast<const f32x4*>(k.sc + c), mu = *reinterpret_cast<const f32x4*>(k.mu + c);
    const f32x4 k1 = *reinterpret_cast<const f32x4*>(k.k1 + c), k2 = *reinterpret_cast<const f32x4*>(k.k2 + c);
#pragma unroll
    for (int e = 0; e < 4; ++e) out[e] = sp_bn_dz1(gy[e], zv[e], s[e], mu[e], k1[e], k2[e]);
    return out;
}

// SuperPointNetBn for the kernels of og_superpoint_train.h: the gradient is dz formed on load, the layer's input sp_bn_act of the raw
// map below (through its pool, where there is one).  The data gradient is that of the input ACTIVATION, stored unmasked: the ReLU mask
// and the pool routing of the layer below are applied where that layer's gy is formed.  No bias gradient.
struct SpBn {
    struct Grad {
        const float *g, *z;          // the gradient of the layer's activation; the layer's raw output
        SpBnCoef k;
    };
    struct In {
        const float *z, *cf;         // the raw map of the layer below [B][Hz][Wz][Cin] and its forward coefficients
        int Hz, Wz;
    };
    static constexpr bool kBias = false, kPoolOnLoad = true, kDump1a = true;
    template <bool POOLED>
    static __device__ __forceinline__ f32x4 grad_at(const Grad& s, int b, int H, int W, int C, int y, int x, int c) {
        return sp_bn_dz<POOLED>(s.g, s.z, s.k, b, H, W, C, y, x, c);
    }
    template <bool INPOOL>
    static __device__ __forceinline__ f32x4 input_at(const In& s, int b, int H, int W, int C, int y, int x, int c) {
        return sp_bn_act_at<INPOOL>(s.z, s.cf, b, s.Hz, s.Wz, C, y, x, c);
    }
    static __device__ __forceinline__ auto grad1a(const Grad& s, int co) {          // bn1a is not pooled
        const float sc = s.k.sc[co], be = s.k.be[co], mu = s.k.mu[co], k1 = s.k.k1[co], k2 = s.k.k2[co];
        return [=, g = s.g, z = s.z](int64_t p) {
            const float zv = z[p * 64 + co];
            const float gy = sp_bn_act(zv, mu, sc, be) > 0.f ? g[p * 64 + co] : 0.f;
            return sp_bn_dz1(gy, zv, sc, mu, k1, k2);
        };
    }
    static __device__ __forceinline__ float dx_value(const In&, int64_t, float v) { return v; }
};

// ---------------------------------------------------------------- forward: conv1a raw, with statistics partials
// Workgroup = SPB_TILE consecutive pixels of B * H * W; thread (c4 = tid & 15, slot = tid >> 4) takes every 16th pixel.
// part [64][T][3] = (pivot, sum (z - pivot), sum (z - pivot)^2) over the tile's valid pixels, pivot = z at the tile's first pixel, the
// 16 slots added in slot order, accumulated in float64 and rounded once.  Sums about a value inside the data do not cancel where
// |mean| >> sigma; on integer data they are exact.
__global__ __launch_bounds__(256) void sp_bn_conv1a_kernel(const float* __restrict__ img, const float* __restrict__ w,
                                                           const float* __restrict__ bias, int B, int H, int W, float* __restrict__ zout,
                                                           float* __restrict__ part) {
    __shared__ double red[16][64][2];
    __shared__ float pivot[64];
    const int tid = threadIdx.x, c4 = (tid & 15) * 4, slot = tid >> 4;
    const int64_t total = (int64_t)B * H * W, p0 = (int64_t)blockIdx.x * SPB_TILE;
    double s1[4] = {0.0, 0.0, 0.0, 0.0}, s2[4] = {0.0, 0.0, 0.0, 0.0};            // ATen's CPU kernel accumulates in double too
    const f32x4 bv = *reinterpret_cast<const f32x4*>(bias + c4);
    f32x4 zs[SPB_TILE / 16];
#pragma unroll
    for (int u = 0; u < SPB_TILE / 16; ++u) {
        const int64_t p = p0 + slot + 16 * u;
        zs[u] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (p >= total) continue;
        const int x = (int)(p % W), y = (int)((p / W) % H);
        const float* im = img + (p / ((int64_t)W * H)) * H * W;
        f32x4 acc = bv;
#pragma unroll
        for (int ky = 0; ky < 3; ++ky)
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) {
                const int yy = y + ky - 1, xx = x + kx - 1;
                const float v = (yy >= 0 && yy < H && xx >= 0 && xx < W) ? im[(int64_t)yy * W + xx] : 0.f;
                const f32x4 wv = *reinterpret_cast<const f32x4*>(w + (ky * 3 + kx) * 64 + c4);
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[e] = __builtin_fmaf(wv[e], v, acc[e]);
            }
        *reinterpret_cast<f32x4*>(zout + p * 64 + c4) = acc;
        zs[u] = acc;
    }
    if (slot == 0) {                                                        // pixel p0 < total: the grid has no empty tile
#pragma unroll
        for (int e = 0; e < 4; ++e) pivot[c4 + e] = zs[0][e];
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < SPB_TILE / 16; ++u) {
        if (p0 + slot + 16 * u >= total) continue;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const double d = (double)(zs[u][e] - pivot[c4 + e]);
            s1[e] += d;
            s2[e] = __builtin_fma(d, d, s2[e]);
        }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        red[slot][c4 + e][0] = s1[e];
        red[slot][c4 + e][1] = s2[e];
    }
    __syncthreads();
    if (tid < 128) {
        const int c = tid >> 1, k = tid & 1;
        double v = 0.0;
#pragma unroll
        for (int s = 0; s < 16; ++s) v += red[s][c][k];
        part[((int64_t)c * gridDim.x + blockIdx.x) * 3 + 1 + k] = (float)v;
        if (k == 0) part[((int64_t)c * gridDim.x + blockIdx.x) * 3] = pivot[c];
    }
}

// ---------------------------------------------------------------- forward: 3x3 convolution of the normalised, activated layer below
// z = conv(act(zin)) + b stored raw at every valid pixel; part [Cout][tiles][3] = (pivot, sum (z - pivot), sum (z - pivot)^2) over the
// tile's valid pixels, pivot = z at the tile's first pixel (as sp_bn_conv1a_kernel): per lane over its accumulator registers in register
// order, the two half-waves, then the two wave rows.
template <int BN, bool INPOOL>
__global__ __launch_bounds__(256, 2) void sp_bn_conv3x3_kernel(const float* __restrict__ zin, const float* __restrict__ cf,
                                                               const float* __restrict__ wp,
                                                               const float* __restrict__ bias, int B, int H, int W, int Hz, int Wz, int Cin,
                                                               int Cout, float* __restrict__ zout, float* __restrict__ part) {
    constexpr int TM = 2, TN = BN / 64;                                    // zin is [B][Hz][Wz][Cin]: this layer's H x W, or twice that behind a pool
    __shared__ __attribute__((aligned(16))) float tile[SP_HALO_H * SP_HALO_W * SP_LDSC];
    __shared__ double red[2][BN][2];
    __shared__ float pivot[BN];
    const SpTile t = sp_tile(H, W, BN);
    const int b = t.b, lane = t.lane;
    f32x16 acc[TM][TN];
    // one accumulator per pass of 32 input channels, as the data gradient: a single fp32 chain over 9 Cin products is ~3x as far from
    // float64 as ATen's blocked sums, and the two-pixel statistics of a small image amplify that tenfold per coarse layer
    sp_conv3x3_accumulate<BN, true>([=](int gy, int gx, int c) { return sp_bn_act_at<INPOOL>(zin, cf, b, Hz, Wz, Cin, gy, gx, c); }, wp, H, W, Cin,
                              t, tile, acc);
    if (t.wm == 0 && lane < 32) {                                           // accumulator register 0 of lanes 0..31: tile pixel (0, 0), always valid
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            const int cl = t.wn * (BN / 2) + j * 32 + lane;
            pivot[cl] = acc[0][j][0] + bias[t.n0 + cl];
        }
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < TN; ++j) {
        const int cl = t.wn * (BN / 2) + j * 32 + (lane & 31);
        const int co = t.n0 + cl;
        const float bv = bias[co], pv = pivot[cl];
        double s1 = 0.0, s2 = 0.0;                                          // double, as ATen's CPU kernel: one rounding per tile partial
#pragma unroll
        for (int i = 0; i < TM; ++i) {
            const int band = t.ty0 + 4 * t.wm + 2 * i;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int m = mfma32_row(r, lane);
                const int y = band + (m >> 4), x = t.tx0 + (m & 15);
                if (y >= H || x >= W) continue;
                const float zv = acc[i][j][r] + bv;
                zout[(((int64_t)b * H + y) * W + x) * Cout + co] = zv;
                const double d = (double)(zv - pv);
                s1 += d;
                s2 = __builtin_fma(d, d, s2);
            }
        }
        s1 += __shfl_xor(s1, 32, 64);
        s2 += __shfl_xor(s2, 32, 64);
        if (lane < 32) {
            red[t.wm][cl][0] = s1;
            red[t.wm][cl][1] = s2;
        }
    }
    __syncthreads();
    for (int f = threadIdx.x; f < BN * 2; f += 256) {
        const int cl = f >> 1, k = f & 1;
        part[((int64_t)(t.n0 + cl) * gridDim.x + blockIdx.x) * 3 + 1 + k] = (float)(red[0][cl][k] + red[1][cl][k]);
        if (k == 0) part[((int64_t)(t.n0 + cl) * gridDim.x + blockIdx.x) * 3] = pivot[cl];
    }
}

// ---------------------------------------------------------------- forward: the statistics of one layer from its tile partials
// One workgroup per channel.  Tile t holds n_t pixels (from the geometry: 8 x 16 tiles cut by the image edge when tiles_x > 0, else flat
// tiles of SPB_TILE pixels of `total`), mean_t = pivot + s1 / n_t, M2_t = s2 - s1^2 / n_t, all in float64.  Thread i merges its contiguous run
// of tiles in tile order, then the 256 runs merge pairwise (i with i + 128, i + 64, ...): (n, mean, M2) <- Chan's update.  Never
// E[z^2] - mean^2 over the whole map.  Channels < split belong to module 0, the rest to module 1 (bnPa | bnDa).
struct SpBnModule {
    const float *gamma, *beta;
    float *running_mean, *running_var;
    float eps, momentum;
};
__device__ __forceinline__ void sp_bn_merge(double& na, double& ma, double& qa, double nb, double mb, double qb) {
    if (nb == 0.0) return;
    const double n = na + nb, d = mb - ma;
    ma = ma + d * (nb / n);
    qa = qa + qb + d * d * (na * nb / n);
    na = n;
}
__global__ __launch_bounds__(256) void sp_bn_stats_finish_kernel(const float* __restrict__ part, int T, int tiles_x, int tiles_y, int H, int W,
                                                                 int64_t total, SpBnModule m0, SpBnModule m1, int split, int C,
                                                                 float* __restrict__ coef) {
    __shared__ double sn[256], sm[256], sq[256];
    const int c = blockIdx.x, tid = threadIdx.x;
    const int per = (T + 255) / 256;
    const int t0 = tid * per, t1 = min(T, t0 + per);
    double n = 0.0, mean = 0.0, q = 0.0;
    for (int t = t0; t < t1; ++t) {
        double nt;
        if (tiles_x > 0) {
            const int tx = t % tiles_x, ty = (t / tiles_x) % tiles_y;
            nt = (double)(min(SP_TH, H - ty * SP_TH) * min(SP_TW, W - tx * SP_TW));
        } else {
            nt = (double)min((int64_t)SPB_TILE, total - (int64_t)t * SPB_TILE);
        }
        const float* pt = part + ((int64_t)c * T + t) * 3;
        const double s1 = (double)pt[1], s2 = (double)pt[2];
        sp_bn_merge(n, mean, q, nt, (double)pt[0] + s1 / nt, fmax(s2 - s1 * (s1 / nt), 0.0));
    }
    sn[tid] = n;
    sm[tid] = mean;
    sq[tid] = q;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) {
            sp_bn_merge(sn[tid], sm[tid], sq[tid], sn[tid + s], sm[tid + s], sq[tid + s]);
        }
        __syncthreads();
    }
    if (tid == 0) {
        const SpBnModule& m = c < split ? m0 : m1;
        const int cm = c < split ? c : c - split;
        const double N = sn[0], mu = sm[0], var = sq[0] / N;
        const double r = 1.0 / sqrt(var + (double)m.eps);
        coef[c] = (float)mu;
        coef[C + c] = (float)r;
        coef[2 * C + c] = (float)((double)m.gamma[cm] * r);
        coef[3 * C + c] = m.beta[cm];
        const double mom = (double)m.momentum;
        m.running_mean[cm] = (float)((1.0 - mom) * (double)m.running_mean[cm] + mom * mu);
        m.running_var[cm] = (float)((1.0 - mom) * (double)m.running_var[cm] + mom * (sq[0] / (N - 1.0)));
    }
}

// the heads' hidden activation at coarse resolution, [npix][512]
__global__ __launch_bounds__(256) void sp_bn_act_kernel(const float* __restrict__ z, const float* __restrict__ cf, int64_t n4, int C,
                                                        float* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n4) return;
    const int c = (int)(i % (C / 4)) * 4;
    const f32x4 v = *reinterpret_cast<const f32x4*>(z + i * 4), u = *reinterpret_cast<const f32x4*>(cf + c);
    const f32x4 s = *reinterpret_cast<const f32x4*>(cf + 2 * C + c), t = *reinterpret_cast<const f32x4*>(cf + 3 * C + c);
    f32x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = sp_bn_act(v[e], u[e], s[e], t[e]);
    *reinterpret_cast<f32x4*>(out + i * 4) = o;
}

// ---------------------------------------------------------------- forward: softmax + depth-to-space and the L2 norm behind bnPb / bnDb
// One wave per coarse cell: logits [npix][ldl] (65 used), draw [npix][256] -> heat [B][Hc*8][Wc*8], desc [npix][256].
__global__ __launch_bounds__(256) void sp_bn_cell_tail_kernel(const float* __restrict__ logits, int64_t ldl, const float* __restrict__ draw,
                                                              int npix, int Hc, int Wc, float* __restrict__ heat, float* __restrict__ desc) {
    const int lane = threadIdx.x & 63;
    const int64_t p = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (p >= npix) return;
    const float l = logits[p * ldl + lane], dust = logits[p * ldl + 64];
    const float mx = fmaxf(wave_max(l), dust);
    const float e = expf(l - mx);
    const float sum = wave_sum(e) + expf(dust - mx);
    const int64_t b = p / ((int64_t)Hc * Wc);
    const int rem = (int)(p - b * Hc * Wc), cy = rem / Wc, cx = rem - cy * Wc;
    heat[(b * Hc * 8 + cy * 8 + (lane >> 3)) * (Wc * 8) + cx * 8 + (lane & 7)] = e / sum;
    f32x4 v = *reinterpret_cast<const f32x4*>(draw + p * SP_D + lane * 4);
    const float nrm = sqrtf(wave_sum(__builtin_fmaf(v[0], v[0], __builtin_fmaf(v[1], v[1], __builtin_fmaf(v[2], v[2], v[3] * v[3])))));
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = v[k] / nrm;
    *reinterpret_cast<f32x4*>(desc + p * SP_D + lane * 4) = v;
}

// ---------------------------------------------------------------- backward: per-tile partials of dbeta and dgamma
// Workgroup = SPB_TILE consecutive pixels of the layer's B * H * W, all C channels: thread (q = tid % (C/4), slot = tid / (C/4)) takes
// every (1024 / C)-th pixel; part [C][T][2] = (sum gy, sum gy (z - mean)), slots added in slot order.
template <bool POOLED>
__global__ __launch_bounds__(256) void sp_bn_reduce_kernel(const float* __restrict__ g, const float* __restrict__ z, SpBnCoef k, int B, int H,
                                                           int W, int C, float* __restrict__ part) {
    __shared__ float red[2048];                                             // [slots][C][2], slots * C = 1024
    const int tid = threadIdx.x, c4n = C / 4, q = tid % c4n, slot = tid / c4n, nslots = 1024 / C;
    const int64_t total = (int64_t)B * H * W, p0 = (int64_t)blockIdx.x * SPB_TILE;
    f32x4 s1{0.f, 0.f, 0.f, 0.f}, s2{0.f, 0.f, 0.f, 0.f};
    for (int i = slot; i < SPB_TILE; i += nslots) {
        const int64_t p = p0 + i;
        if (p >= total) break;
        const int x = (int)(p % W), y = (int)((p / W) % H), b = (int)(p / ((int64_t)W * H));
        f32x4 gy, zv;
        sp_bn_gy<POOLED>(g, z, k, b, H, W, C, y, x, q * 4, gy, zv);
        const f32x4 mu = *reinterpret_cast<const f32x4*>(k.mu + q * 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            s1[e] += gy[e];
            s2[e] = __builtin_fmaf(gy[e], zv[e] - mu[e], s2[e]);
        }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        red[(slot * C + q * 4 + e) * 2] = s1[e];
        red[(slot * C + q * 4 + e) * 2 + 1] = s2[e];
    }
    __syncthreads();
    for (int f = tid; f < 2 * C; f += 256) {
        const int c = f >> 1, kk = f & 1;
        float v = 0.f;
        for (int s = 0; s < nslots; ++s) v += red[(s * C + c) * 2 + kk];
        part[((int64_t)c * gridDim.x + blockIdx.x) * 2 + kk] = v;
    }
}

// One workgroup per channel: the partials in float64, thread runs in tile order, then pairwise.  dbeta = S_g, dgamma = rstd S_g(z - mean);
// kb = k1 | k2 for sp_bn_dz1.
__global__ __launch_bounds__(256) void sp_bn_reduce_finish_kernel(const float* __restrict__ part, int T, double N, const float* __restrict__ coef,
                                                                  int C, float* __restrict__ dgamma, float* __restrict__ dbeta,
                                                                  float* __restrict__ kb) {
    __shared__ double sa[256], sb[256];
    const int c = blockIdx.x, tid = threadIdx.x;
    const int per = (T + 255) / 256;
    const int t0 = tid * per, t1 = min(T, t0 + per);
    double a = 0.0, b = 0.0;
    for (int t = t0; t < t1; ++t) {
        a += (double)part[((int64_t)c * T + t) * 2];
        b += (double)part[((int64_t)c * T + t) * 2 + 1];
    }
    sa[tid] = a;
    sb[tid] = b;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) {
            sa[tid] += sa[tid + s];
            sb[tid] += sb[tid + s];
        }
        __syncthreads();
    }
    if (tid == 0) {
        const double r = (double)coef[C + c];
        const double db = sa[0], dg = r * sb[0];
        dbeta[c] = (float)db;
        dgamma[c] = (float)dg;
        kb[c] = (float)(db / N);
        kb[C + c] = (float)(r * dg / N);
    }
}

// ---------------------------------------------------------------- host side
// Saved (floats): hidden [npix][512] activated first, so that the caller can view it; the forward coefficients of the nine layers
// (4 C each); z1a; z[j] of the eight MFMA layers at the resolution they convolve at.
struct BnSaved {
    int64_t hidden, coef, z1a, z[SP_LAYERS], total;
};
BnSaved bn_saved_layout(int B, int H, int W) {
    BnSaved S{};
    int64_t o = 0;
    auto take = [&](int64_t n) {
        const int64_t at = o;
        o += og_round_up(n, 64);
        return at;
    };
    const Dims d = dims(H, W);
    S.hidden = take((int64_t)B * d.Hc * d.Wc * 512);
    S.coef = take(4 * SPB_CHANNELS);
    S.z1a = take((int64_t)B * H * W * 64);
    for (int j = 0; j < SP_LAYERS; ++j) {
        int h, w;
        layer_dims(j, H, W, h, w);
        S.z[j] = take((int64_t)B * h * w * kCout[j]);
    }
    S.total = o;
    return S;
}

int flat_tiles(int B, int h, int w) { return (int)(((int64_t)B * h * w + SPB_TILE - 1) / SPB_TILE); }

// Workspace (floats), forward and backward: the statistics [C][T][3] / reduction [C][T][2] partials of the largest layer, the backward
// coefficients k1 | k2, the two data-gradient buffers and the weight-gradient partials.
struct BnWs {
    int64_t stat, kb;
    BackwardWs bwd;
};
BnWs bn_ws_layout(int B, int H, int W) {
    BnWs w{};
    int64_t stat = (int64_t)64 * flat_tiles(B, H, W) * 3;
    for (int j = 0; j < SP_LAYERS; ++j) {
        int h, ww;
        layer_dims(j, H, W, h, ww);
        stat = std::max(stat, (int64_t)kCout[j] * std::max(conv_tiles(B, h, ww), flat_tiles(B, h, ww)) * 3);
    }
    w.stat = 0;
    w.kb = og_round_up(stat, 64);
    w.bwd = backward_layout(w.kb + og_round_up(2 * 512, 64), B, H, W, false);
    return w;
}

bool bn_shape_ok(int B, int H, int W) { return dense_shape_ok(B, H, W) && (int64_t)B * (H / 8) * (W / 8) >= 2; }

// modules: bn1a, bn1b, ..., bn4b, bnPa, bnDa; layer L < 8 is module L, layer 8 is modules 8 | 9
void stats_finish(const float* part, int T, int tiles_x, int tiles_y, int h, int w, int64_t total, int L, float* const* bn, const float* eps,
                  const float* momentum, float* coef, hipStream_t st) {
    auto module = [&](int m) { return SpBnModule{bn[4 * m], bn[4 * m + 1], bn[4 * m + 2], bn[4 * m + 3], eps[m], momentum[m]}; };
    const int C = kBnC[L];
    const SpBnModule m0 = module(L), m1 = module(L == 8 ? 9 : L);
    hipLaunchKernelGGL(sp_bn_stats_finish_kernel, dim3(C), dim3(256), 0, st, part, T, tiles_x, tiles_y, h, w, total, m0, m1, L == 8 ? 256 : C, C,
                       coef + 4 * bn_offset(L));
}

template <int BN, bool INPOOL>
void bn_conv(const float* zin, const float* cf, const float* w, const float* bias, int B, int H, int W, int Hz, int Wz,
             int Cin, int Cout, float* zout, float* part, hipStream_t st) {
    hipLaunchKernelGGL((sp_bn_conv3x3_kernel<BN, INPOOL>), dim3(conv_tiles(B, H, W), Cout / BN), dim3(256), 0, st, zin, cf, w, bias, B, H, W,
                       Hz, Wz, Cin, Cout, zout, part);
}

// what backward_layers asks of the network.  grad: dbeta, dgamma (into bn_grads) and the backward coefficients of BatchNorm layer L from
// the gradient g of its activation, launched ahead of the layer's kernels, which then form dz on load.
struct BnBackward {
    int B, H, W;
    const float* A;                                  // the saved buffer
    BnSaved S;
    float *stat, *kb, *bn_grads;
    hipStream_t st;
    SpBn::Grad grad(int L, const float* g, int h, int w) const {
        const int C = kBnC[L], T = flat_tiles(B, h, w), o = bn_offset(L);
        const float* z = L == 0 ? A + S.z1a : A + S.z[L - 1];
        const float* cf = A + S.coef + 4 * o;
        const SpBnCoef k = bn_coef(cf, nullptr, C);
        if (L > 0 && kPooled[L - 1]) hipLaunchKernelGGL(sp_bn_reduce_kernel<true>, dim3(T), dim3(256), 0, st, g, z, k, B, h, w, C, stat);
        else hipLaunchKernelGGL(sp_bn_reduce_kernel<false>, dim3(T), dim3(256), 0, st, g, z, k, B, h, w, C, stat);
        hipLaunchKernelGGL(sp_bn_reduce_finish_kernel, dim3(C), dim3(256), 0, st, stat, T, (double)B * h * w, cf, C, bn_grads + o,
                           bn_grads + SPB_CHANNELS + o, kb);
        return {g, z, bn_coef(cf, kb, C)};
    }
    SpBn::In input(int j) const {                    // the raw map below layer j, at the resolution it was convolved at, and its coefficients
        int hz = H, wz = W;
        if (j > 0) layer_dims(j - 1, H, W, hz, wz);
        return {j == 0 ? A + S.z1a : A + S.z[j - 1], A + S.coef + 4 * bn_offset(j), hz, wz};
    }
};

}  // namespace

extern "C" size_t og_superpoint_bn_train_saved_bytes(int32_t batch, int32_t H, int32_t W) {
    if (!bn_shape_ok(batch, H, W)) return 0;
    return (size_t)bn_saved_layout(batch, H, W).total * 4;
}

extern "C" size_t og_superpoint_bn_train_workspace_bytes(int32_t batch, int32_t H, int32_t W) {
    if (!bn_shape_ok(batch, H, W)) return 0;
    return (size_t)bn_ws_layout(batch, H, W).bwd.total * 4 + 256;
}

extern "C" int og_superpoint_bn_train_forward(int32_t batch, int32_t H, int32_t W, const float* image, const void* packed_dev,
                                              float* const* bn, const float* eps, const float* momentum, void* saved_dev,
                                              void* workspace_dev, void* stream) {
    og_clear_status();
    if (!image || !packed_dev || !bn || !eps || !momentum || !saved_dev || !workspace_dev) return OG_E_INVALID;
    for (int i = 0; i < 40; ++i)
        if (!bn[i]) return OG_E_INVALID;
    if (!bn_shape_ok(batch, H, W)) return OG_E_SHAPE;
    if ((uintptr_t)packed_dev % 16 || (uintptr_t)saved_dev % 16 || (uintptr_t)workspace_dev % 16) return OG_E_ALIGN;
    const SpLayout L = sp_layout();
    const float* P = (const float*)packed_dev;
    const BnSaved S = bn_saved_layout(batch, H, W);
    const BnWs Wk = bn_ws_layout(batch, H, W);
    float* A = (float*)saved_dev;
    float* coef = A + S.coef;
    float* part = (float*)workspace_dev + Wk.stat;
    hipStream_t st = (hipStream_t)stream;

    const int T1 = flat_tiles(batch, H, W);
    hipLaunchKernelGGL(sp_bn_conv1a_kernel, dim3(T1), dim3(256), 0, st, image, P + L.w1a, P + L.b1a, batch, H, W, A + S.z1a, part);
    stats_finish(part, T1, 0, 0, H, W, (int64_t)batch * H * W, 0, bn, eps, momentum, coef, st);
    for (int j = 0; j < SP_LAYERS; ++j) {
        int h, w, hz = H, wz = W;
        layer_dims(j, H, W, h, w);
        if (j > 0) layer_dims(j - 1, H, W, hz, wz);
        const bool inpool = j > 0 && kPooled[j - 1];
        const float* zin = j == 0 ? A + S.z1a : A + S.z[j - 1];
        const float* cin = coef + 4 * bn_offset(j);                          // the layer below is BatchNorm layer j
        const int Cin = kCin[j], Cout = kCout[j];
        if (Cout == 64) {
            if (inpool) bn_conv<64, true>(zin, cin, P + L.w[j], P + L.b[j], batch, h, w, hz, wz, Cin, Cout, A + S.z[j], part, st);
            else bn_conv<64, false>(zin, cin, P + L.w[j], P + L.b[j], batch, h, w, hz, wz, Cin, Cout, A + S.z[j], part, st);
        } else {
            if (inpool) bn_conv<128, true>(zin, cin, P + L.w[j], P + L.b[j], batch, h, w, hz, wz, Cin, Cout, A + S.z[j], part, st);
            else bn_conv<128, false>(zin, cin, P + L.w[j], P + L.b[j], batch, h, w, hz, wz, Cin, Cout, A + S.z[j], part, st);
        }
        stats_finish(part, conv_tiles(batch, h, w), (w + SP_TW - 1) / SP_TW, (h + SP_TH - 1) / SP_TH, h, w, (int64_t)batch * h * w, j + 1, bn, eps,
                     momentum, coef, st);
    }
    const Dims d = dims(H, W);
    const int64_t n4 = (int64_t)batch * d.Hc * d.Wc * 128;
    const float* c8 = coef + 4 * bn_offset(8);
    hipLaunchKernelGGL(sp_bn_act_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, st, A + S.z[7], c8, n4, 512,
                       A + S.hidden);
    return og_launch_status();
}

extern "C" int og_superpoint_bn_cell_tail(int32_t batch, int32_t Hc, int32_t Wc, const float* logits, int64_t ld_logits, const float* desc_raw,
                                          float* heatmap, float* coarse_desc, void* stream) {
    og_clear_status();
    if (batch <= 0 || Hc <= 0 || Wc <= 0 || ld_logits < 65 || (int64_t)batch * Hc * Wc > (1ll << 20)) return OG_E_SHAPE;
    if (!logits || !desc_raw || !heatmap || !coarse_desc) return OG_E_INVALID;
    if ((uintptr_t)desc_raw % 16 || (uintptr_t)coarse_desc % 16) return OG_E_ALIGN;
    const int npix = batch * Hc * Wc;
    hipLaunchKernelGGL(sp_bn_cell_tail_kernel, dim3((npix + 3) / 4), dim3(256), 0, (hipStream_t)stream, logits, ld_logits, desc_raw, npix, Hc, Wc,
                       heatmap, coarse_desc);
    return og_launch_status();
}

extern "C" int og_superpoint_bn_train_backward(int32_t batch, int32_t H, int32_t W, const float* image, const void* packed_grad_dev,
                                               const void* saved_dev, const float* g_hidden, int32_t first_layer, float* grads,
                                               float* bn_grads, float* layer_grads, void* workspace_dev, void* stream) {
    og_clear_status();
    if (!image || !packed_grad_dev || !saved_dev || !g_hidden || !grads || !bn_grads || !workspace_dev) return OG_E_INVALID;
    if (!bn_shape_ok(batch, H, W) || first_layer < 0 || first_layer > SP_LAYERS) return OG_E_SHAPE;
    if ((uintptr_t)packed_grad_dev % 16 || (uintptr_t)saved_dev % 16 || (uintptr_t)g_hidden % 16 || (uintptr_t)workspace_dev % 16 ||
        (uintptr_t)layer_grads % 16)
        return OG_E_ALIGN;
    const BnWs Wk = bn_ws_layout(batch, H, W);
    float* ws = (float*)workspace_dev;
    BnBackward net{batch, H, W, (const float*)saved_dev, bn_saved_layout(batch, H, W), ws + Wk.stat, ws + Wk.kb, bn_grads, (hipStream_t)stream};
    // grads: as og_superpoint_train_backward; the bias slots are left untouched
    backward_layers<SpBn>(net, batch, H, W, image, (const float*)packed_grad_dev, g_hidden, first_layer, grads, layer_grads, ws, Wk.bwd,
                          (hipStream_t)stream);
    return og_launch_status();
}
