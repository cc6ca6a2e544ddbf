// SuperPointNet fine-tuning: the training forward (which keeps what the backward needs) and the backward of the extractor, exact fp32
// on v_mfma_f32_32x32x2_f32, no atomics: every sum has a fixed order, so the gradients are bit-identical from run to run.
// (reference models/matching_module.py:29-31,77 `finetune: True`; models/features/superpoint/model.py SuperPointNet.forward.)
//
// Layers: conv1a (VALU) and the eight 3x3 MFMA layers j = 0..7 of og_superpoint_dense.h (conv1b, 2a, 2b, 3a, 3b, 4a, 4b, heads Pa | Da);
// j = 0, 2, 4 end in the 2x2 max-pool.  G_j is the gradient of layer j's pre-activation output, stored at the resolution of the
// layer's OUTPUT: for a pooled layer that is the pooled map, and the full-resolution gradient is formed on load (sp_grad_at: the
// pooled value goes to the first maximum of its window in raster order, torch's rule; rows / columns the pool dropped get 0).
//
//   forward      the inference kernels, except that the pooled layers also store their activation before the pool
//                (sp_conv3x3_save_kernel).  Saved: the post-ReLU output of every 3x3 layer, pooled and unpooled.
//   dgrad        G_{j-1} = (3x3 convolution of G_j with the weights transposed and the taps flipped) masked by x_j > 0: the K loop of
//                the forward kernel with a second packed blob, G_j read through sp_grad_at, the ReLU mask of the layer below in the
//                store; every pass of 32 channels x 9 taps is summed on its own and then added to the total (K is up to 9 x 512).
//   wgrad        dW[co][ci][tap] = sum over pixels of G[p][co] x[p + tap][ci]: a workgroup owns a 32 x 32 (co, ci) block and all nine
//                taps over a contiguous range of 8 x 16 pixel tiles (split-K over pixels); per tile dy [128][32] and the x halo
//                [180][32] are staged in LDS, each wave takes two tile rows as 16 k-steps x 9 taps of MFMA.  The waves are summed in
//                wave order, the splits by sp_reduce_parts_kernel in split order.  The bias gradient is the sum of the A operands.
//   wgrad1a      conv1a has one input channel: 64 x 9 sums over all pixels on the VALU, same two stages.
//   describe     backward of sample_desc_from_points + F.normalize: one wave per keypoint writes dv, its cell and its four weights;
//                then one wave per coarse cell gathers from the keypoints that touch it, in keypoint order.
// dgrad, wgrad, wgrad1a, the dump kernel and the loop over the layers live in og_superpoint_train.h, which SuperPointNetBn runs too;
// this unit instantiates them with the policy SpPlain.
#include "og_superpoint_train.h"

namespace {

// ---------------------------------------------------------------- forward of a pooled layer that also keeps the unpooled activation
// out = pool(relu(conv + b)) exactly as sp_conv3x3_kernel<BN, true> (max over the window, then bias and ReLU); pre = relu(conv + b) at
// every pixel.  Rounding is monotone, so the maximum of the four `pre` values of a window equals `out` bit for bit: comparing `pre`
// values finds the pool's argmax.
template <int BN>
__global__ __launch_bounds__(256, 2) void sp_conv3x3_save_kernel(const float* __restrict__ in, const float* __restrict__ wp,
                                                                 const float* __restrict__ bias, int B, int H, int W, int Cin, int Cout,
                                                                 float* __restrict__ out, float* __restrict__ pre) {
    constexpr int TM = 2, TN = BN / 64;
    __shared__ __attribute__((aligned(16))) float tile[SP_HALO_H * SP_HALO_W * SP_LDSC];
    const SpTile t = sp_tile(H, W, BN);
    const int b = t.b, lane = t.lane;
    const float* inb = in + (int64_t)b * H * W * Cin;
    f32x16 acc[TM][TN];
    sp_conv3x3_accumulate<BN>([=](int gy, int gx, int c) { return *reinterpret_cast<const f32x4*>(inb + ((int64_t)gy * W + gx) * Cin + c); },
                              wp, H, W, Cin, t, tile, acc);
    const int Hp = H / 2, Wp = W / 2;
#pragma unroll
    for (int j = 0; j < TN; ++j) {
        const int co = t.n0 + t.wn * (BN / 2) + j * 32 + (lane & 31);
        const float bv = bias[co];
#pragma unroll
        for (int i = 0; i < TM; ++i) {
            const int band = t.ty0 + 4 * t.wm + 2 * i;              // first image row of this MFMA tile
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int m = mfma32_row(r, lane);
                const int y = band + (m >> 4), x = t.tx0 + (m & 15);
                if (y < H && x < W) pre[(((int64_t)b * H + y) * W + x) * Cout + co] = fmaxf(acc[i][j][r] + bv, 0.f);
            }
            const int py = band / 2;
            if (py >= Hp) continue;
#pragma unroll
            for (int r = 0; r < 8; r += 2) {
                const int m = mfma32_row(r, lane);                  // even column, upper row of the window
                const int px = (t.tx0 + (m & 15)) / 2;
                if (px >= Wp) continue;
                float v = fmaxf(fmaxf(acc[i][j][r], acc[i][j][r + 1]), fmaxf(acc[i][j][r + 8], acc[i][j][r + 9]));
                v = fmaxf(v + bv, 0.f);
                out[(((int64_t)b * Hp + py) * Wp + px) * Cout + co] = v;
            }
        }
    }
}

// ---------------------------------------------------------------- the gradient of a layer's pre-activation output at pixel (y, x)
// Channels c .. c + 3 of image b.  !POOLED: g is [B][H][W][C] as it lies.  POOLED: g is [B][H/2][W/2][C], the gradient of the pooled
// map (already masked by pooled > 0), and a [B][H][W][C] the activation before the pool: the pixel receives the window's gradient iff
// it is the first of the window's four pixels, in raster order, that holds the maximum.  A pixel outside every window (the last row /
// column of an odd size) receives exactly 0.  Pixel (y, x) must be inside the image.
template <bool POOLED>
__device__ __forceinline__ f32x4 sp_grad_at(const float* __restrict__ g, const float* __restrict__ a, int b, int H, int W, int C, int y,
                                            int x, int c) {
    if constexpr (!POOLED) {
        return *reinterpret_cast<const f32x4*>(g + (((int64_t)b * H + y) * W + x) * C + c);
    } else {
        const int Hp = H / 2, Wp = W / 2, py = y >> 1, px = x >> 1;
        f32x4 out{0.f, 0.f, 0.f, 0.f};
        if (py >= Hp || px >= Wp) return out;
        const float* a0 = a + (((int64_t)b * H + 2 * py) * W + 2 * px) * C + c;        // rows 2 py, 2 py + 1 < H; columns 2 px, 2 px + 1 < W
        const f32x4 a00 = *reinterpret_cast<const f32x4*>(a0), a01 = *reinterpret_cast<const f32x4*>(a0 + C);
        const f32x4 a10 = *reinterpret_cast<const f32x4*>(a0 + (int64_t)W * C), a11 = *reinterpret_cast<const f32x4*>(a0 + (int64_t)W * C + C);
        const f32x4 gv = *reinterpret_cast<const f32x4*>(g + (((int64_t)b * Hp + py) * Wp + px) * C + c);
        const int me = (y & 1) * 2 + (x & 1);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float m = fmaxf(fmaxf(a00[e], a01[e]), fmaxf(a10[e], a11[e]));
            const int win = a00[e] == m ? 0 : a01[e] == m ? 1 : a10[e] == m ? 2 : 3;
            out[e] = win == me ? gv[e] : 0.f;
        }
        return out;
    }
}

// SuperPointNet for the kernels of og_superpoint_train.h: G through sp_grad_at, the layer's input as it was saved (post-ReLU), the data
// gradient masked by that input > 0, and a bias gradient.
struct SpPlain {
    struct Grad {
        const float *g, *a;          // the gradient at the layer's output resolution; the activation before the pool (pooled layers)
    };
    struct In {
        const float* x;
    };
    static constexpr bool kBias = true, kPoolOnLoad = false, kDump1a = false;
    template <bool POOLED>
    static __device__ __forceinline__ f32x4 grad_at(const Grad& s, int b, int H, int W, int C, int y, int x, int c) {
        return sp_grad_at<POOLED>(s.g, s.a, b, H, W, C, y, x, c);
    }
    template <bool INPOOL>
    static __device__ __forceinline__ f32x4 input_at(const In& s, int b, int H, int W, int C, int y, int x, int c) {
        return *reinterpret_cast<const f32x4*>(s.x + (((int64_t)b * H + y) * W + x) * C + c);
    }
    static __device__ __forceinline__ auto grad1a(const Grad& s, int co) {
        return [g = s.g, co](int64_t p) { return g[p * 64 + co]; };
    }
    static __device__ __forceinline__ float dx_value(const In& s, int64_t o, float v) { return s.x[o] > 0.f ? v : 0.f; }
};

// ---------------------------------------------------------------- backward of describe (bilinear sample + F.normalize)
// The four taps of a keypoint, as sp_describe_kernel computes them: cell (y0, x0) and its right / lower neighbours, weights nw ne sw se.
__device__ __forceinline__ void sp_sample_taps(int idx, int Hc, int Wc, int& x0, int& y0, float (&w)[4]) {
    const int Wh = Wc * 8, Hh = Hc * 8;
    const float x = (float)(idx % Wh), y = (float)(idx / Wh);
    const float gx = (x - 4.f + 0.5f) / ((float)Wh - 4.5f) * 2.f - 1.f;
    const float gy = (y - 4.f + 0.5f) / ((float)Hh - 4.5f) * 2.f - 1.f;
    const float ix = ((gx + 1.f) * Wc - 1.f) / 2.f, iy = ((gy + 1.f) * Hc - 1.f) / 2.f;
    const float fx = floorf(ix), fy = floorf(iy);
    x0 = (int)fx;
    y0 = (int)fy;
    const float x1 = (float)(x0 + 1), y1 = (float)(y0 + 1);
    w[0] = (x1 - ix) * (y1 - iy);
    w[1] = (ix - fx) * (y1 - iy);
    w[2] = (x1 - ix) * (iy - fy);
    w[3] = (ix - fx) * (iy - fy);
}

// one wave per keypoint: v = sum of w_i d[cell_i], out = v / max(|v|, 1e-12); dv = (dout - out (out . dout)) / max(|v|, 1e-12).
// kcell [B][n][2] = (x0, y0), kw [B][n][4] = the weights, dv [B][n][256].
__global__ __launch_bounds__(256) void sp_describe_bwd_point_kernel(int Hc, int Wc, int n, const int32_t* __restrict__ sidx, int64_t sel_ld,
                                                                    const float* __restrict__ cdesc, const float* __restrict__ dout,
                                                                    int32_t* __restrict__ kcell, float* __restrict__ kw, float* __restrict__ dv) {
    const int lane = threadIdx.x & 63;
    const int k = blockIdx.x * 4 + (threadIdx.x >> 6), b = blockIdx.y;
    if (k >= n) return;
    int x0, y0;
    float w[4];
    sp_sample_taps(sidx[b * sel_ld + k], Hc, Wc, x0, y0, w);
    const int64_t o = (int64_t)b * n + k;
    if (lane == 0) {
        kcell[o * 2] = x0;
        kcell[o * 2 + 1] = y0;
    }
    if (lane < 4) kw[o * 4 + lane] = w[lane];
    const float* db = cdesc + (int64_t)b * Hc * Wc * SP_D + lane * 4;
    f32x4 v{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int yy = y0 + (i >> 1), xx = x0 + (i & 1);
        if (yy < 0 || yy >= Hc || xx < 0 || xx >= Wc) continue;
        const f32x4 d = *reinterpret_cast<const f32x4*>(db + ((int64_t)yy * Wc + xx) * SP_D);
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = fmaf(d[e], w[i], v[e]);
    }
    const float nrm = fmaxf(sqrtf(wave_sum(v[0] * v[0] + v[1] * v[1] + v[2] * v[2] + v[3] * v[3])), 1e-12f);
    const f32x4 go = *reinterpret_cast<const f32x4*>(dout + o * SP_D + lane * 4);
    float dot = 0.f;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        v[e] = v[e] / nrm;
        dot = fmaf(v[e], go[e], dot);
    }
    dot = wave_sum(dot);
    f32x4 r;
#pragma unroll
    for (int e = 0; e < 4; ++e) r[e] = (go[e] - v[e] * dot) / nrm;
    *reinterpret_cast<f32x4*>(dv + o * SP_D + lane * 4) = r;
}

// one wave per coarse cell: the gradient of the (normalised) coarse descriptor, gathered from the keypoints that touch the cell, in
// keypoint order -- no atomics, the same bits from run to run
__global__ __launch_bounds__(64) void sp_describe_bwd_cell_kernel(int Hc, int Wc, int n, const int32_t* __restrict__ kcell,
                                                                  const float* __restrict__ kw, const float* __restrict__ dv,
                                                                  float* __restrict__ dcoarse) {
    const int lane = threadIdx.x, cell = blockIdx.x, b = blockIdx.y;
    const int cy = cell / Wc, cx = cell - cy * Wc;
    f32x4 acc{0.f, 0.f, 0.f, 0.f};
    const int2* kc = reinterpret_cast<const int2*>(kcell) + (int64_t)b * n;
    // 64 keypoints per step: every lane tests one, then the wave walks the few that touch the cell, lowest keypoint first
    for (int k0 = 0; k0 < n; k0 += 64) {
        bool hit = false;
        if (k0 + lane < n) {
            const int2 c = kc[k0 + lane];
            hit = (unsigned)(cx - c.x) <= 1u && (unsigned)(cy - c.y) <= 1u;
        }
        unsigned long long m = __ballot(hit);
        while (m) {
            const int k = k0 + __ffsll((long long)m) - 1;
            m &= m - 1;
            const int64_t o = (int64_t)b * n + k;
            const int2 c = kc[k];
            const float w = kw[o * 4 + (cy - c.y) * 2 + (cx - c.x)];
            const f32x4 d = *reinterpret_cast<const f32x4*>(dv + o * SP_D + lane * 4);
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[e] = fmaf(w, d[e], acc[e]);
        }
    }
    *reinterpret_cast<f32x4*>(dcoarse + ((int64_t)b * Hc * Wc + cell) * SP_D + lane * 4) = acc;
}

// ---------------------------------------------------------------- host side
// Saved activations (floats), hidden first so that the caller can view it: A8 hidden [Hc][512]; A0 conv1a; then per layer j its
// output act[j] (pooled for the pooled layers) and, for the pooled layers, pre[j] before the pool.
struct Saved {
    int64_t hidden, a1a, act[SP_LAYERS - 1], pre[SP_LAYERS - 1], total;
};
Saved saved_layout(int B, int H, int W) {
    Saved S{};
    int64_t o = 0;
    auto take = [&](int64_t n) {
        const int64_t at = o;
        o += og_round_up(n, 64);
        return at;
    };
    const Dims d = dims(H, W);
    S.hidden = take((int64_t)B * d.Hc * d.Wc * 512);
    S.a1a = take((int64_t)B * H * W * 64);
    for (int j = 0; j < SP_LAYERS - 1; ++j) {
        int h, w;
        layer_dims(j, H, W, h, w);
        if (kPooled[j]) {
            S.pre[j] = take((int64_t)B * h * w * kCout[j]);
            S.act[j] = take((int64_t)B * (h / 2) * (w / 2) * kCout[j]);
        } else {
            S.act[j] = take((int64_t)B * h * w * kCout[j]);
        }
    }
    S.total = o;
    return S;
}

template <int BN>
void conv_save(const float* in, const float* w, const float* bias, int B, int H, int W, int Cin, int Cout, float* out, float* pre,
               hipStream_t st) {
    hipLaunchKernelGGL((sp_conv3x3_save_kernel<BN>), dim3(conv_tiles(B, H, W), Cout / BN), dim3(256), 0, st, in, w, bias, B, H, W, Cin, Cout,
                       out, pre);
}

// what backward_layers asks of the network: G of a layer as the chain hands it over, routed through the saved pre-pool activation
struct PlainBackward {
    const float* A;
    Saved S;
    SpPlain::Grad grad(int L, const float* g, int, int) const { return {g, L > 0 && kPooled[L - 1] ? A + S.pre[L - 1] : nullptr}; }
    SpPlain::In input(int j) const { return {j == 0 ? A + S.a1a : A + S.act[j - 1]}; }
};

}  // namespace

extern "C" size_t og_superpoint_train_packed_bytes(int32_t descriptor_dim) {
    if (descriptor_dim != SP_D) return 0;
    return (size_t)dgrad_offset(SP_LAYERS) * 4;
}

extern "C" int og_superpoint_train_pack(int32_t descriptor_dim, const float* const* params, void* packed_host) {
    if (descriptor_dim != SP_D) return OG_E_SHAPE;
    if (!params || !packed_host) return OG_E_INVALID;
    for (int i = 0; i < 24; ++i)
        if (!params[i]) return OG_E_INVALID;
    float* P = (float*)packed_host;
    bool finite = true;
    auto put = [&](int64_t o, double v) {
        const float f = (float)v;
        finite = finite && std::isfinite(f);
        P[o] = f;
    };
    for (int j = 0; j < SP_LAYERS; ++j) {
        const int Cin = kCin[j], Cout = kCout[j];
        // rows = the layer's INPUT channels, K = 9 taps x the layer's OUTPUT channels, tap t of the blob = tap 8 - t of the weight
        pack_fragments(put, dgrad_offset(j), Cin, Cin, 9 * Cout, [&](int ci, int k) {
            int co, tap;
            conv3x3_k(k, SP_KC, co, tap);
            const int conv = j < 7 ? j + 1 : (co < 256 ? 8 : 10);         // heads: convPa rows 0..255, convDa rows 256..511
            return (double)params[2 * conv][((int64_t)(co % 256) * Cin + ci) * 9 + (8 - tap)];
        });
    }
    return finite ? 0 : OG_E_RANGE;
}

extern "C" size_t og_superpoint_train_saved_bytes(int32_t batch, int32_t H, int32_t W) {
    if (!dense_shape_ok(batch, H, W)) return 0;
    return (size_t)saved_layout(batch, H, W).total * 4;
}

extern "C" size_t og_superpoint_train_workspace_bytes(int32_t batch, int32_t H, int32_t W, int32_t n) {
    if (!dense_shape_ok(batch, H, W) || n < 0) return 0;
    const size_t bwd = (size_t)backward_layout(0, batch, H, W, true).total * 4;
    const size_t desc = (size_t)og_round_up((int64_t)batch * n * (SP_D + 8) * 4, 256);
    return std::max(bwd, desc) + 256;
}

extern "C" int og_superpoint_train_forward(int32_t batch, int32_t H, int32_t W, const float* image, const void* packed_dev, void* saved_dev,
                                           float* heatmap, float* coarse_desc, void* stream) {
    og_clear_status();
    if (!image || !packed_dev || !saved_dev || !heatmap || !coarse_desc) return OG_E_INVALID;
    if (!dense_shape_ok(batch, H, W)) return OG_E_SHAPE;
    if ((uintptr_t)packed_dev % 16 || (uintptr_t)coarse_desc % 16 || (uintptr_t)saved_dev % 16) return OG_E_ALIGN;
    const SpLayout L = sp_layout();
    const float* P = (const float*)packed_dev;
    const Dims d = dims(H, W);
    const Saved S = saved_layout(batch, H, W);
    float* A = (float*)saved_dev;
    hipStream_t st = (hipStream_t)stream;
    const int64_t n1a = (int64_t)batch * H * W * 16;
    hipLaunchKernelGGL(sp_conv1a_kernel, dim3((unsigned)((n1a + 255) / 256)), dim3(256), 0, st, image, P + L.w1a, P + L.b1a, batch, H, W, A + S.a1a);
    conv_save<64>(A + S.a1a, P + L.w[0], P + L.b[0], batch, H, W, 64, 64, A + S.act[0], A + S.pre[0], st);                    // conv1b + pool
    conv<64, false>(A + S.act[0], P + L.w[1], P + L.b[1], batch, d.H2, d.W2, 64, 64, A + S.act[1], st);                      // conv2a
    conv_save<64>(A + S.act[1], P + L.w[2], P + L.b[2], batch, d.H2, d.W2, 64, 64, A + S.act[2], A + S.pre[2], st);          // conv2b + pool
    conv<128, false>(A + S.act[2], P + L.w[3], P + L.b[3], batch, d.H4, d.W4, 64, 128, A + S.act[3], st);                    // conv3a
    conv_save<128>(A + S.act[3], P + L.w[4], P + L.b[4], batch, d.H4, d.W4, 128, 128, A + S.act[4], A + S.pre[4], st);       // conv3b + pool
    conv<128, false>(A + S.act[4], P + L.w[5], P + L.b[5], batch, d.Hc, d.Wc, 128, 128, A + S.act[5], st);                   // conv4a
    conv<128, false>(A + S.act[5], P + L.w[6], P + L.b[6], batch, d.Hc, d.Wc, 128, 128, A + S.act[6], st);                   // conv4b
    conv<128, false>(A + S.act[6], P + L.w[7], P + L.b[7], batch, d.Hc, d.Wc, 128, 512, A + S.hidden, st);                   // convPa | convDa
    const int npix = batch * d.Hc * d.Wc;
    hipLaunchKernelGGL(sp_cell_kernel, dim3((npix + SP_CELL_PIX - 1) / SP_CELL_PIX), dim3(256), 0, st, A + S.hidden, P + L.wc, P + L.bc, npix,
                       d.Hc, d.Wc, heatmap, coarse_desc);
    return og_launch_status();
}

extern "C" int og_superpoint_train_backward(int32_t batch, int32_t H, int32_t W, const float* image, const void* packed_grad_dev,
                                            const void* saved_dev, const float* g_hidden, int32_t first_layer, float* grads,
                                            float* layer_grads, void* workspace_dev, void* stream) {
    og_clear_status();
    if (!image || !packed_grad_dev || !saved_dev || !g_hidden || !grads || !workspace_dev) return OG_E_INVALID;
    if (!dense_shape_ok(batch, H, W) || first_layer < 0 || first_layer > SP_LAYERS) return OG_E_SHAPE;
    if ((uintptr_t)packed_grad_dev % 16 || (uintptr_t)saved_dev % 16 || (uintptr_t)g_hidden % 16 || (uintptr_t)workspace_dev % 16 ||
        (uintptr_t)layer_grads % 16)
        return OG_E_ALIGN;
    PlainBackward net{(const float*)saved_dev, saved_layout(batch, H, W)};
    backward_layers<SpPlain>(net, batch, H, W, image, (const float*)packed_grad_dev, g_hidden, first_layer, grads, layer_grads,
                             (float*)workspace_dev, backward_layout(0, batch, H, W, true), (hipStream_t)stream);
    return og_launch_status();
}

extern "C" int og_superpoint_describe_backward(int32_t batch, int32_t Hc, int32_t Wc, int32_t n, const int32_t* sel_idx, int64_t sel_ld,
                                               const float* coarse_desc, const float* d_descriptors, float* d_coarse, void* workspace_dev,
                                               void* stream) {
    og_clear_status();
    if (batch <= 0 || Hc <= 0 || Wc <= 0 || n <= 0 || sel_ld < n || (int64_t)batch * Hc * Wc > (1ll << 20)) return OG_E_SHAPE;
    if (!sel_idx || !coarse_desc || !d_descriptors || !d_coarse || !workspace_dev) return OG_E_INVALID;
    if ((uintptr_t)coarse_desc % 16 || (uintptr_t)d_descriptors % 16 || (uintptr_t)d_coarse % 16 || (uintptr_t)workspace_dev % 16) return OG_E_ALIGN;
    hipStream_t st = (hipStream_t)stream;
    float* dv = (float*)workspace_dev;                                       // [B][n][256] | kw [B][n][4] | kcell [B][n][2]
    float* kw = dv + (int64_t)batch * n * SP_D;
    int32_t* kcell = (int32_t*)(kw + (int64_t)batch * n * 4);
    hipLaunchKernelGGL(sp_describe_bwd_point_kernel, dim3((n + 3) / 4, batch), dim3(256), 0, st, Hc, Wc, n, sel_idx, sel_ld, coarse_desc,
                       d_descriptors, kcell, kw, dv);
    hipLaunchKernelGGL(sp_describe_bwd_cell_kernel, dim3(Hc * Wc, batch), dim3(64), 0, st, Hc, Wc, n, kcell, kw, dv, d_coarse);
    return og_launch_status();
}
