// SuperPoint detector + descriptor, inference only (reference models/features/superpoint/model.py, superpoint/utils.py,
// models/features/utils.py:26-51 min_stack).  Exact fp32 throughout: the convolutions run on v_mfma_f32_32x32x2_f32, the
// selection is a pure comparison of fp32 heatmap values, so the path is deterministic.
//
// Layout: activations NHWC fp32.  Stages (og_superpoint_dense / _detect / _describe, include/openglue_amd.h); the kernels of the dense
// stage (conv1a, conv3x3, cell) live in og_superpoint_dense.h, which superpoint_train.hip includes as well:
//   conv1a       1 -> 64, VALU, one thread per (pixel, 4 channels)                                  full resolution
//   conv3x3      implicit GEMM: a workgroup owns 8 x 16 output pixels x BN channels; the input tile and its 1-pixel halo
//                are staged in LDS 32 channels at a time, the K loop runs over 9 taps x 32 channels reading A fragments at
//                tap offsets (no im2col buffer); weights are packed fragment-major (pack_fragments of og_conv_f32.h, shared with
//                patchnet.hip) with BatchNorm folded.  Epilogue: bias,
//                ReLU and, for conv{1,2,3}b, the 2x2 max-pool (floor semantics), so the unpooled map is never stored.
//                convPa and convDa run as one launch with 512 output channels.
//   cell         convPb (65) and convDb (D) on the 512-channel hidden map: softmax over 65, dustbin dropped, depth-to-space
//                into the heatmap [B][Hc*8][Wc*8]; descriptor divided by its L2 norm (no eps) into [B][Hc][Wc][D].
//   nms          kornia nms2d restated: replicate padding by (k-1)/2, a pixel is kept only when STRICTLY greater than the
//                maximum of its k*k-1 neighbours (centre excluded); plus F.threshold (> thr, != 0) and remove_borders.
//                Per (row, 256-column segment) counts, an exclusive scan per image, then compaction in raster order
//                (block_exclusive_scan_inplace and block_rank_of of og_block.h).
//   select       top_k_keypoints + min_stack on device: each candidate's rank under the key (score desc, raster index asc)
//                is counted exactly, so the selection is identical from run to run and ties go to the lower raster index.
//   describe     sample_desc_from_points (grid_sample bilinear, align_corners=False, zero padding) + F.normalize, LAFs, scores.
#include "og_superpoint_dense.h"

namespace {

constexpr int SP_NMS_SEG = 256;                      // columns per NMS segment
constexpr int SP_NMS_RMAX = 8;                       // nms_kernel <= 17

// ---------------------------------------------------------------- NMS + threshold + borders, segment counts
// Workgroup (segment, row, image): 256 columns of one heatmap row; LDS holds rows y - r .. y + r of columns x0 - r .. x0 + 255 + r,
// coordinates clamped into the image (replicate padding).  mask[b][y][x] = 1 for a candidate; seg[b][y * nseg + s] = its count.
__global__ __launch_bounds__(256) void sp_nms_kernel(const float* __restrict__ heat, int Hh, int Wh, int rad, int border, float thr,
                                                     uint8_t* __restrict__ mask, int32_t* __restrict__ seg) {
    __shared__ float t[2 * SP_NMS_RMAX + 1][SP_NMS_SEG + 2 * SP_NMS_RMAX];
    const int nseg = (Wh + SP_NMS_SEG - 1) / SP_NMS_SEG;
    const int s = blockIdx.x, y = blockIdx.y, b = blockIdx.z;
    const int x0 = s * SP_NMS_SEG, tid = threadIdx.x;
    const float* hb = heat + (int64_t)b * Hh * Wh;
    const int rows = 2 * rad + 1, cols = SP_NMS_SEG + 2 * rad;
    for (int f = tid; f < rows * cols; f += 256) {
        const int rr = f / cols, cc = f - rr * cols;
        const int yy = min(max(y - rad + rr, 0), Hh - 1), xx = min(max(x0 - rad + cc, 0), Wh - 1);
        t[rr][cc] = hb[(int64_t)yy * Wh + xx];
    }
    __syncthreads();
    const int x = x0 + tid;
    int keep = 0;
    if (x < Wh) {
        const float v = t[rad][tid + rad];
        float mx = OG_NEG_INF;
        for (int dy = 0; dy < rows; ++dy)
            for (int dx = 0; dx < rows; ++dx)
                if (dy != rad || dx != rad) mx = fmaxf(mx, t[dy][tid + dx]);
        keep = v > mx && v > thr && v != 0.f && x >= border && x < Wh - border && y >= border && y < Hh - border;
        mask[((int64_t)b * Hh + y) * Wh + x] = (uint8_t)keep;
    }
    const int cnt = __syncthreads_count(keep);
    if (tid == 0) seg[((int64_t)b * Hh + y) * nseg + s] = cnt;
}

// exclusive scan of one image's segment counts (raster order), total -> counts[b]
__global__ __launch_bounds__(256) void sp_scan_kernel(int32_t* __restrict__ seg, int nseg_img, int32_t* __restrict__ counts) {
    block_exclusive_scan_inplace(seg + (int64_t)blockIdx.x * nseg_img, nseg_img, counts + blockIdx.x);
}

// candidates of one segment written at its scanned offset, in column order: cand_idx = y * Wh + x, cand_score = heat
__global__ __launch_bounds__(256) void sp_compact_kernel(const float* __restrict__ heat, const uint8_t* __restrict__ mask, int Hh, int Wh,
                                                         const int32_t* __restrict__ seg, int64_t cap, int32_t* __restrict__ cidx,
                                                         float* __restrict__ cscore) {
    __shared__ int wsum[4];
    const int nseg = (Wh + SP_NMS_SEG - 1) / SP_NMS_SEG;
    const int s = blockIdx.x, y = blockIdx.y, b = blockIdx.z;
    const int x = s * SP_NMS_SEG + (int)threadIdx.x;
    const int64_t pix = ((int64_t)b * Hh + y) * Wh + x;
    const bool keep = x < Wh && mask[pix];
    int cnt;
    const int rank = block_rank_of(keep, wsum, cnt);
    if (!keep) return;
    const int off = seg[((int64_t)b * Hh + y) * nseg + s] + rank;
    cidx[b * cap + off] = y * Wh + x;
    cscore[b * cap + off] = heat[pix];
}

// top_k_keypoints + min_stack.  Per image: c_b = n_b if k < 0 or k >= n_b else k; m = min_b c_b.  If every c_b is equal each image
// keeps c_b -- in raster order when it was not cut (c_b == n_b), else its c_b best by descending score; otherwise every image keeps
// its m best by descending score (min_stack's torch.topk runs on every image, the smallest included).  The rank of candidate i is
// the number of candidates j with (score_j, -index_j) > (score_i, -index_i): exact, distinct, independent of scheduling.
__global__ __launch_bounds__(256) void sp_select_kernel(const int32_t* __restrict__ counts_in, int B, int max_kpts, int64_t cap,
                                                        const int32_t* __restrict__ cidx, const float* __restrict__ cscore, int64_t sel_ld,
                                                        int32_t* __restrict__ counts_out, int32_t* __restrict__ sidx, float* __restrict__ sscore) {
    __shared__ float ss[256];
    __shared__ int32_t si[256];
    const int b = blockIdx.y, tid = threadIdx.x;
    int cmin = 0x7fffffff, cfirst = -1;
    bool equal = true;
    for (int i = 0; i < B; ++i) {
        const int n = counts_in[i];
        const int c = (max_kpts < 0 || max_kpts >= n) ? n : max_kpts;
        if (cfirst < 0) cfirst = c;
        equal = equal && c == cfirst;
        cmin = min(cmin, c);
    }
    const int n = counts_in[b];
    const int cb = (max_kpts < 0 || max_kpts >= n) ? n : max_kpts;
    const int m = equal ? cb : cmin;
    const bool raster = equal && cb == n;
    if (blockIdx.x == 0 && tid == 0) {
        counts_out[b] = n;
        counts_out[B + b] = m;
    }
    const int64_t i = (int64_t)blockIdx.x * 256 + tid;
    if ((int64_t)blockIdx.x * 256 >= n) return;
    const int32_t* ci = cidx + b * cap;
    const float* cs = cscore + b * cap;
    const bool live = i < n;
    const float v = live ? cs[i] : 0.f;
    const int32_t vi = live ? ci[i] : 0;
    if (raster) {
        if (live && i < m) {
            sidx[b * sel_ld + i] = vi;
            sscore[b * sel_ld + i] = v;
        }
        return;
    }
    int rank = 0;
    for (int j0 = 0; j0 < n; j0 += 256) {
        __syncthreads();
        if (j0 + tid < n) {
            ss[tid] = cs[j0 + tid];
            si[tid] = ci[j0 + tid];
        }
        __syncthreads();
        const int lim = min(256, n - j0);
        for (int j = 0; j < lim; ++j) {
            const float u = ss[j];
            rank += (u > v) || (u == v && si[j] < vi);
        }
    }
    if (live && rank < m) {
        sidx[b * sel_ld + rank] = vi;
        sscore[b * sel_ld + rank] = v;
    }
}

// one wave per keypoint: LAF, score, bilinear descriptor (grid_sample, align_corners=False, zero padding) and F.normalize
__global__ __launch_bounds__(256) void sp_describe_kernel(int B, int Hc, int Wc, int n, const int32_t* __restrict__ sidx,
                                                          const float* __restrict__ sscore, int64_t sel_ld, const float* __restrict__ cdesc,
                                                          float* __restrict__ lafs, float* __restrict__ scores, float* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int k = blockIdx.x * 4 + (threadIdx.x >> 6), b = blockIdx.y;
    if (k >= n) return;
    const int Wh = Wc * 8, Hh = Hc * 8;
    const int idx = sidx[b * sel_ld + k];
    const float x = (float)(idx % Wh), y = (float)(idx / Wh);
    const int64_t o = (int64_t)b * n + k;
    if (lane == 0) {
        float* L = lafs + o * 6;
        L[0] = 1.f; L[1] = 0.f; L[2] = x;
        L[3] = 0.f; L[4] = 1.f; L[5] = y;
        scores[o] = sscore[b * sel_ld + k];
    }
    // sample_desc_from_points: (p - cell/2 + 0.5) / (size - cell/2 - 0.5) * 2 - 1, then grid_sample's unnormalisation
    const float gx = (x - 4.f + 0.5f) / ((float)Wh - 4.5f) * 2.f - 1.f;
    const float gy = (y - 4.f + 0.5f) / ((float)Hh - 4.5f) * 2.f - 1.f;
    const float ix = ((gx + 1.f) * Wc - 1.f) / 2.f, iy = ((gy + 1.f) * Hc - 1.f) / 2.f;
    const float fx = floorf(ix), fy = floorf(iy);
    const int x0 = (int)fx, y0 = (int)fy, x1 = x0 + 1, y1 = y0 + 1;
    const float w_nw = ((float)x1 - ix) * ((float)y1 - iy), w_ne = (ix - fx) * ((float)y1 - iy);
    const float w_sw = ((float)x1 - ix) * (iy - fy), w_se = (ix - fx) * (iy - fy);
    const float* db = cdesc + (int64_t)b * Hc * Wc * SP_D + lane * 4;
    f32x4 v{0.f, 0.f, 0.f, 0.f};
    auto tap = [&](int yy, int xx, float w) {
        if (yy < 0 || yy >= Hc || xx < 0 || xx >= Wc) return;
        const f32x4 d = *reinterpret_cast<const f32x4*>(db + ((int64_t)yy * Wc + xx) * SP_D);
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = fmaf(d[e], w, v[e]);
    };
    tap(y0, x0, w_nw);
    tap(y0, x1, w_ne);
    tap(y1, x0, w_sw);
    tap(y1, x1, w_se);
    const float ss = wave_sum(v[0] * v[0] + v[1] * v[1] + v[2] * v[2] + v[3] * v[3]);
    const float nrm = fmaxf(sqrtf(ss), 1e-12f);
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = v[e] / nrm;
    *reinterpret_cast<f32x4*>(out + o * SP_D + lane * 4) = v;
}

// ---------------------------------------------------------------- host side
int64_t sp_capacity(int Hh, int Wh, int max_kpts) {
    // a candidate is strictly greater than its 8 neighbours (nms_kernel >= 3): at most one per 2x2 block
    const int64_t cap = (int64_t)((Hh + 1) / 2) * ((Wh + 1) / 2);
    return max_kpts > 0 && max_kpts < cap ? max_kpts : cap;
}

struct DetectWs {
    uint8_t* mask;
    int32_t* seg;
    int32_t* cand_idx;
    float* cand_score;
    int32_t* counts;
    size_t bytes;
};
DetectWs detect_layout(void* base, int B, int Hh, int Wh) {
    const int64_t cap = sp_capacity(Hh, Wh, -1);
    const int nseg = (Wh + SP_NMS_SEG - 1) / SP_NMS_SEG;
    char* p = (char*)base;
    size_t o = 0;
    DetectWs w{};
    w.mask = (uint8_t*)(p + o); o += og_round_up((int64_t)B * Hh * Wh, 256);
    w.seg = (int32_t*)(p + o); o += og_round_up((int64_t)B * Hh * nseg * 4, 256);
    w.cand_idx = (int32_t*)(p + o); o += og_round_up((int64_t)B * cap * 4, 256);
    w.cand_score = (float*)(p + o); o += og_round_up((int64_t)B * cap * 4, 256);
    w.counts = (int32_t*)(p + o); o += og_round_up((int64_t)B * 4, 256);
    w.bytes = o;
    return w;
}
size_t dense_bytes(int B, int H, int W) {
    const Dims d = dims(H, W);
    return og_round_up((int64_t)B * H * W * 64 * 4, 256) + og_round_up((int64_t)B * d.H2 * d.W2 * 64 * 4, 256);
}

double fold_scale(const float* const* bn, int c, double eps) { return (double)bn[0][c] / std::sqrt((double)bn[3][c] + eps); }

}  // namespace

extern "C" size_t og_superpoint_packed_bytes(int32_t descriptor_dim) {
    if (descriptor_dim != SP_D) return 0;
    return (size_t)sp_layout().total * 4;
}

// params: 24 host pointers, the weight and bias of conv1a, conv1b, ..., conv4b, convPa, convPb, convDa, convDb; with batch_norm
// 48 more, weight / bias / running_mean / running_var of bn1a, ..., bn4b, bnPa, bnPb, bnDa, bnDb.
extern "C" int og_superpoint_pack(int32_t descriptor_dim, int32_t batch_norm, float bn_eps, const float* const* params, void* packed_host) {
    if (descriptor_dim != SP_D) return OG_E_SHAPE;
    if (!params || !packed_host) return OG_E_INVALID;
    const int nconv = 12;
    for (int i = 0; i < nconv * 2 + (batch_norm ? nconv * 4 : 0); ++i)
        if (!params[i]) return OG_E_INVALID;
    const SpLayout L = sp_layout();
    float* P = (float*)packed_host;
    bool finite = true;
    // folded weight / bias of conv i, output channel co: W * s, (b - mean) * s + beta
    auto scale = [&](int i, int co) -> double { return batch_norm ? fold_scale(params + nconv * 2 + i * 4, co, bn_eps) : 1.0; };
    auto shift = [&](int i, int co) -> double {
        const double b = params[2 * i + 1][co];
        if (!batch_norm) return b;
        const float* const* bn = params + nconv * 2 + i * 4;
        return (b - bn[2][co]) * scale(i, co) + bn[1][co];
    };
    auto put = [&](int64_t o, double v) {
        const float f = (float)v;
        finite = finite && std::isfinite(f);
        P[o] = f;
    };
    // conv1a: [tap][64]
    for (int co = 0; co < 64; ++co) {
        for (int t = 0; t < 9; ++t) put(L.w1a + t * 64 + co, (double)params[0][co * 9 + t] * scale(0, co));
        put(L.b1a + co, shift(0, co));
    }
    // 3x3 convs, fragment-major; heads: convPa (conv 8) rows 0..255, convDa (conv 10) rows 256..511
    for (int l = 0; l < 8; ++l) {
        const int Cin = kCin[l], Cout = kCout[l];
        auto conv_of = [l](int co) { return l < 7 ? l + 1 : (co < 256 ? 8 : 10); };
        for (int co = 0; co < Cout; ++co) put(L.b[l] + co, shift(conv_of(co), co % 256));
        pack_fragments(put, L.w[l], Cout, Cout, 9 * Cin, [&](int co, int k) {
            int ci, tap;
            conv3x3_k(k, SP_KC, ci, tap);
            return (double)params[2 * conv_of(co)][((int64_t)(co % 256) * Cin + ci) * 9 + tap] * scale(conv_of(co), co % 256);
        });
    }
    // cell: tiles 0..2 convPb (conv 9, 65 rows, zero-padded to 96), tiles 3..10 convDb (conv 11)
    for (int row = 0; row < 32 * SP_P_TILES; ++row) put(L.bc + row, row < 65 ? shift(9, row) : 0.0);
    for (int row = 0; row < SP_D; ++row) put(L.bc + 32 * SP_P_TILES + row, shift(11, row));
    pack_fragments(put, L.wc, 65, 32 * SP_P_TILES, 256, [&](int row, int k) { return (double)params[18][row * 256 + k] * scale(9, row); });
    pack_fragments(put, L.wc + (int64_t)SP_P_TILES * 32 * 256, SP_D, SP_D, 256,
                   [&](int row, int k) { return (double)params[22][row * 256 + k] * scale(11, row); });
    return finite ? 0 : OG_E_RANGE;
}

extern "C" int og_superpoint_capacity(int32_t H, int32_t W, int32_t max_kpts) {
    if (H < 8 || W < 8) return 0;
    return (int)sp_capacity(H / 8 * 8, W / 8 * 8, max_kpts);
}

extern "C" size_t og_superpoint_workspace_bytes(int32_t batch, int32_t H, int32_t W, int32_t nms_kernel, int32_t max_kpts) {
    (void)nms_kernel;
    (void)max_kpts;
    if (!dense_shape_ok(batch, H, W)) return 0;
    const size_t det = detect_layout(nullptr, batch, H / 8 * 8, W / 8 * 8).bytes;
    const size_t den = dense_bytes(batch, H, W);
    return det > den ? det : den;
}

extern "C" int og_superpoint_dense(int32_t batch, int32_t H, int32_t W, const float* image, const void* packed_dev, float* heatmap,
                                   float* coarse_desc, void* workspace_dev, void* stream) {
    og_clear_status();
    if (!image || !packed_dev || !heatmap || !coarse_desc || !workspace_dev) return OG_E_INVALID;
    if (!dense_shape_ok(batch, H, W)) return OG_E_SHAPE;
    if ((uintptr_t)packed_dev % 16 || (uintptr_t)coarse_desc % 16 || (uintptr_t)workspace_dev % 16) return OG_E_ALIGN;
    const SpLayout L = sp_layout();
    const float* P = (const float*)packed_dev;
    const Dims d = dims(H, W);
    hipStream_t st = (hipStream_t)stream;
    float* X = (float*)workspace_dev;
    float* Y = (float*)((char*)workspace_dev + og_round_up((int64_t)batch * H * W * 64 * 4, 256));
    const int64_t n1a = (int64_t)batch * H * W * 16;
    hipLaunchKernelGGL(sp_conv1a_kernel, dim3((unsigned)((n1a + 255) / 256)), dim3(256), 0, st, image, P + L.w1a, P + L.b1a, batch, H, W, X);
    conv<64, true>(X, P + L.w[0], P + L.b[0], batch, H, W, 64, 64, Y, st);             // conv1b + pool
    conv<64, false>(Y, P + L.w[1], P + L.b[1], batch, d.H2, d.W2, 64, 64, X, st);      // conv2a
    conv<64, true>(X, P + L.w[2], P + L.b[2], batch, d.H2, d.W2, 64, 64, Y, st);       // conv2b + pool
    conv<128, false>(Y, P + L.w[3], P + L.b[3], batch, d.H4, d.W4, 64, 128, X, st);    // conv3a
    conv<128, true>(X, P + L.w[4], P + L.b[4], batch, d.H4, d.W4, 128, 128, Y, st);    // conv3b + pool
    conv<128, false>(Y, P + L.w[5], P + L.b[5], batch, d.Hc, d.Wc, 128, 128, X, st);   // conv4a
    conv<128, false>(X, P + L.w[6], P + L.b[6], batch, d.Hc, d.Wc, 128, 128, Y, st);   // conv4b
    conv<128, false>(Y, P + L.w[7], P + L.b[7], batch, d.Hc, d.Wc, 128, 512, X, st);   // convPa | convDa
    const int npix = batch * d.Hc * d.Wc;
    hipLaunchKernelGGL(sp_cell_kernel, dim3((npix + SP_CELL_PIX - 1) / SP_CELL_PIX), dim3(256), 0, st, X, P + L.wc, P + L.bc, npix, d.Hc, d.Wc,
                       heatmap, coarse_desc);
    return og_launch_status();
}

extern "C" int og_superpoint_detect(int32_t batch, int32_t Hh, int32_t Wh, int32_t nms_kernel, int32_t border, float threshold,
                                    int32_t max_kpts, const float* heatmap, int32_t* counts, int32_t* sel_idx, float* sel_score,
                                    int64_t sel_ld, void* workspace_dev, void* stream) {
    og_clear_status();
    if (!heatmap || !counts || !sel_idx || !sel_score || !workspace_dev) return OG_E_INVALID;
    if (batch <= 0 || Hh < 8 || Wh < 8 || Hh % 8 || Wh % 8 || (int64_t)batch * Hh * Wh > (1ll << 26)) return OG_E_SHAPE;
    if (nms_kernel < 3 || nms_kernel % 2 == 0 || (nms_kernel - 1) / 2 > SP_NMS_RMAX || border < 0 || max_kpts < -1) return OG_E_SHAPE;
    if (sel_ld < sp_capacity(Hh, Wh, max_kpts)) return OG_E_INVALID;
    if ((uintptr_t)workspace_dev % 16) return OG_E_ALIGN;
    hipStream_t st = (hipStream_t)stream;
    const DetectWs w = detect_layout(workspace_dev, batch, Hh, Wh);
    const int64_t cap = sp_capacity(Hh, Wh, -1);
    const int nseg = (Wh + SP_NMS_SEG - 1) / SP_NMS_SEG;
    const dim3 grid(nseg, Hh, batch);
    hipLaunchKernelGGL(sp_nms_kernel, grid, dim3(256), 0, st, heatmap, Hh, Wh, (nms_kernel - 1) / 2, border, threshold, w.mask, w.seg);
    hipLaunchKernelGGL(sp_scan_kernel, dim3(batch), dim3(256), 0, st, w.seg, Hh * nseg, w.counts);
    hipLaunchKernelGGL(sp_compact_kernel, grid, dim3(256), 0, st, heatmap, w.mask, Hh, Wh, w.seg, cap, w.cand_idx, w.cand_score);
    hipLaunchKernelGGL(sp_select_kernel, dim3((unsigned)((cap + 255) / 256), batch), dim3(256), 0, st, w.counts, batch, max_kpts, cap,
                       w.cand_idx, w.cand_score, sel_ld, counts, sel_idx, sel_score);
    return og_launch_status();
}

extern "C" int og_superpoint_describe(int32_t batch, int32_t Hc, int32_t Wc, int32_t n, const int32_t* sel_idx, const float* sel_score,
                                      int64_t sel_ld, const float* coarse_desc, float* lafs, float* scores, float* descriptors, void* stream) {
    og_clear_status();
    if (batch <= 0 || Hc <= 0 || Wc <= 0 || n < 0 || sel_ld < n) return OG_E_SHAPE;
    if (n == 0) return 0;
    if (!sel_idx || !sel_score || !coarse_desc || !lafs || !scores || !descriptors) return OG_E_INVALID;
    if ((uintptr_t)coarse_desc % 16 || (uintptr_t)descriptors % 16) return OG_E_ALIGN;
    hipLaunchKernelGGL(sp_describe_kernel, dim3((n + 3) / 4, batch), dim3(256), 0, (hipStream_t)stream, batch, Hc, Wc, n, sel_idx, sel_score,
                       sel_ld, coarse_desc, lafs, scores, descriptors);
    return og_launch_status();
}
