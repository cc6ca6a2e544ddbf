// Launch plan of the q | k | v projection: which kernel family serves a request, over which rows and columns.  Plain C++ (no HIP type), so
// that a host-only program can include it (tests/test_proj_plan_cpu.py compiles one).  og_forward* (api.hip) and the stage entry
// og_proj_block (mlp_fused.hip) describe a request, og_proj_plan() turns it into at most OG_PROJ_MAX_STEPS launches, og_launch_proj()
// (mlp_fused.hip) executes one step.  DESIGN.md ("q | k | v projection: the launch plan") holds the table of the rules.
//
//   OG_PROJ_SMALL      proj_small_kernel  (mlp_fused.hip)          columns in output blocks of 32
//   OG_PROJ_WSTAT      proj_wstat_kernel  (proj_wstat.hip)         ... in slabs of 256
//   OG_PROJ_STREAM     proj_stream_kernel (mlp_fused.hip)          ... in groups of 128, at most 8 (the bias area holds 1024 columns); plane rows of whole 128-byte lines
//   OG_PROJ_GEMM       the split-f16 tile GEMM (gemm_f16x3.hip)    ... in channels; with split_row the row-split 256-tile launch
#pragma once
#include <stdint.h>
#include "../../include/openglue_amd.h"      // OG_E_ALIGN, OG_E_SHAPE

enum { OG_PROJ_SMALL = 0, OG_PROJ_WSTAT, OG_PROJ_STREAM, OG_PROJ_GEMM };
enum { OG_PROJ_FORWARD = 0, OG_PROJ_STAGE_ENTRY };        // the two policies: og_forward*'s measured choices / og_proj_block's "every kernel reachable"
constexpr int OG_PROJ_MAX_STEPS = 4;
// What a family cannot take, whoever asks: column unit, token rows per workgroup (a row split falls between two), the low bits of ldy and of the plane
// addresses that must be zero, the widest range in units.  All: K = 256 (128 too, but for WSTAT), fewer than 2^30 rows (32-bit row indices).
constexpr struct { int unit, tile, ldy_mask, plane_mask, widest; } OG_PROJ_FAMILY[4] = {
    {32, 32, 3, 7, 1 << 30}, {256, 32, 7, 15, 1 << 30}, {128, 128, 63, 127, 8}, {1, 1, 0, 0, 1 << 30}};

struct OgProjKnobs { int proj_small, proj_stream, gemm_row_split, gemm_tile, gemm_big2; };      // og_knobs.h values, as the accessors return them

struct OgProjRequest {
    int64_t row0, rows, split;        // token rows [row0, row0 + rows) of X and of the planes; split > 0: the rows below row0 + split take [a0, a1)
    int a0, a1, b0, b1;               // column ranges in channels (= rows of the packed matrix); every other row takes [b0, b1).  og_forward*: a0 == 0, split < rows
    int K, N, relu_cols;              // input channels; width of the packed matrix; favor_relu: the columns below relu_cols carry the feature map's ReLU (else 0)
    bool ragged, has_small, has_big;  // a ragged batch; which fragment-major copies of the matrix exist (og_pack_proj_stream, og_pack_proj_stream_big)
    int64_t ldy; unsigned plane_bits; // leading dimension of the planes, halves; low address bits of both planes, or-ed (the plan adds the byte offset of row0)
    OgProjKnobs knobs;
};

struct OgProjStep {
    int family, relu;                 // relu: OG_PROJ_GEMM only
    int64_t row0; int rows;           // token rows of the launch
    int split_row, a0, a1, b0, b1;    // relative to row0, as the kernels take it; column ranges in the family's unit
};

struct OgProjPlan { int n; OgProjStep step[OG_PROJ_MAX_STEPS]; };

// OG_PROJ_FAMILY applied to a step -- by the plan (to choose) and by og_launch_proj (to refuse): 0, OG_E_ALIGN or OG_E_SHAPE.
inline int og_proj_step_check(const OgProjStep& s, int K, int64_t ldy, unsigned plane_bits) {
    const auto& f = OG_PROJ_FAMILY[s.family];
    if (s.family == OG_PROJ_GEMM) return 0;
    if ((ldy & f.ldy_mask) || (plane_bits & f.plane_mask)) return OG_E_ALIGN;
    const bool ok = (K == 256 || (K == 128 && s.family != OG_PROJ_WSTAT)) && s.rows < (1 << 30) && s.a0 >= 0 && s.b0 >= 0 && s.a1 >= s.a0 && s.b1 >= s.b0 &&
                    s.a1 - s.a0 <= f.widest && s.b1 - s.b0 <= f.widest && !(s.split_row > 0 && s.split_row < s.rows && s.split_row % f.tile) &&
                    (s.family != OG_PROJ_WSTAT || ldy >= 256 * (int64_t)(s.a1 > s.b1 ? s.a1 : s.b1));
    return ok ? 0 : OG_E_SHAPE;
}

// The request as one launch of `family`: false when its ranges are not whole units or og_proj_step_check refuses it (s is filled anyway).
inline bool og_proj_step_for(int family, const OgProjRequest& q, OgProjStep& s) {
    const int u = OG_PROJ_FAMILY[family].unit;
    const int64_t rows = q.rows < ((int64_t)1 << 30) ? q.rows : (int64_t)1 << 30;
    s = OgProjStep{family, q.b0 < q.relu_cols, q.row0, (int)rows, (int)q.split, q.a0 / u, q.a1 / u, q.b0 / u, q.b1 / u};
    if (q.a0 % u || q.a1 % u || q.b0 % u || q.b1 % u) return false;
    return og_proj_step_check(s, q.K, q.ldy, q.plane_bits | (unsigned)((q.row0 * q.ldy * 2) & 127)) == 0;
}

// A row-split launch of the tile GEMM (rows below split_row produce the columns below split_n only) must end up on the second-generation
// 256-tile kernel with at least 192 of the tiles it really computes.  The part of og_gemm_f16x3_row_split_ok that M, N, the split and the
// knobs decide (gemm_f16x3.hip adds what its GemmHArgs say: split-f16 output only, one plain problem).
inline bool og_gemm_row_split_fits(int64_t M, int N, int64_t split_row, int split_n, const OgProjKnobs& k) {
    const int BIG = 256;
    if (split_row <= 0 || split_row >= M || split_row % BIG || split_n <= 0 || split_n >= N || split_n % BIG || M % BIG || N % BIG) return false;
    const int64_t blocks = split_row / BIG * (split_n / BIG) + (M - split_row) / BIG * (N / BIG);
    return k.gemm_row_split && blocks >= 192 && k.gemm_tile != 128 && k.gemm_big2;
}

// The launches that serve a request, in launch order (at most OG_PROJ_MAX_STEPS), behind those p already holds.
//
// OG_PROJ_FORWARD (og_forward*, the measured choices): few rows (<= 8192 per launch; OG_PROJ_SMALL forces) take proj_small_kernel.  Uniform 256-d
// batches take proj_wstat_kernel from 8 units (32-token block x slab) per workgroup on -- 2048 units, the smallest launch it was measured at: a
// workgroup first loads 256 KB of weights, which a run of a few blocks does not pay back.  128-d batches take proj_stream_kernel (OG_PROJ_STREAM
// = 0 / 1 forces it off / on for both widths, 2: at K = 256 only launches that produce every column for all their rows); 256-d batches keep the
// tile GEMMs over it.  A split request that fits no kernel as one launch is one launch on the row-split GEMM (or, from 2048 units on, on
// proj_wstat_kernel) when og_gemm_row_split_fits, else two requests.  What is left is a tile GEMM; with favor_relu a range that spans the
// feature and the value blocks is two of them (ReLU / none).
// OG_PROJ_STAGE_ENTRY (og_proj_block, every kernel reachable whatever og_forward* prefers): above 8192 rows proj_wstat_kernel where the planes
// are as wide as the matrix (og_forward's own geometry) and OG_PROJ_STREAM is unset, else proj_stream_kernel at either width (OG_PROJ_STREAM = 0 /
// non-zero forces it off / on); proj_small_kernel takes the rest -- never a GEMM: what it cannot take, og_launch_proj refuses.
inline OgProjPlan og_proj_plan(const OgProjRequest& q, int policy, OgProjPlan p = OgProjPlan{}) {
    const OgProjKnobs& k = q.knobs;
    const bool fwd = policy == OG_PROJ_FORWARD, favor = q.relu_cols > 0, split = q.split > 0;
    const int64_t R = q.rows, below = split ? q.split : 0;
    const int64_t units = below / 32 * ((q.a1 - q.a0) / 256) + (R - below + 31) / 32 * ((q.b1 - q.b0) / 256);
    const bool row_split = split && !favor && !q.ragged && R < ((int64_t)1 << 30) && q.a0 == 0 && q.b0 == 0 && q.b1 == q.N &&
                           og_gemm_row_split_fits(R, q.N, q.split, q.a1, k);
    const bool small = q.has_small && !favor && (k.proj_small >= 0 ? k.proj_small != 0 : R <= 8192);
    const bool wstat = fwd ? q.has_small && !favor && !q.ragged && q.K == 256 && R > 8192 && units >= 2048 && (!split || row_split)
                           : k.proj_stream < 0 && q.K == 256 && R > 8192 && q.ldy == q.N;
    const bool forced = k.proj_stream > 0 && !(fwd && k.proj_stream == 2), whole = !split && q.b0 == 0 && q.b1 == q.N;
    const bool stream = q.has_big && !favor && k.proj_stream != 0 &&
                        (forced || (R > 8192 && (!fwd || q.K == 128 || (k.proj_stream == 2 && whole))));
    OgProjStep s;
    auto take = [&](int family) { const bool fits = og_proj_step_for(family, q, s); if (fits) p.step[p.n++] = s; return fits; };
    auto part = [&](int64_t row0, int64_t rows, int c0, int c1) {      // rows [row0, row0 + rows) x columns [c0, c1) as a request of its own
        OgProjRequest h = q;
        h.row0 = row0; h.rows = rows; h.split = 0; h.a0 = h.a1 = 0; h.b0 = c0; h.b1 = c1;
        p = og_proj_plan(h, policy, p);
    };
    if (p.n >= OG_PROJ_MAX_STEPS) return p;
    if (fwd && small && take(OG_PROJ_SMALL)) return p;
    if (!(fwd && split) && wstat && take(OG_PROJ_WSTAT)) return p;      // (a split request of og_forward* asks the stream kernel first)
    if (stream && take(OG_PROJ_STREAM)) return p;
    if (!fwd) { og_proj_step_for(OG_PROJ_SMALL, q, s); p.step[p.n++] = s; return p; }
    if (row_split) { if (!(wstat && take(OG_PROJ_WSTAT))) take(OG_PROJ_GEMM); return p; }      // the same one launch on either kernel
    // two launches: the rows from the split on first (the cross layer: image 1's q | k | v, then image 0's q); the feature blocks, then the value block
    if (split) { part(q.row0 + q.split, R - q.split, q.b0, q.b1); part(q.row0, q.split, q.a0, q.a1); }
    else if (q.b0 < q.relu_cols && q.relu_cols < q.b1) { part(q.row0, R, q.b0, q.relu_cols); part(q.row0, R, q.relu_cols, q.b1); }
    else if (q.b1 > q.b0) take(OG_PROJ_GEMM);
    return p;
}
