// The OG_* environment knobs: the single table of them, and the only file of csrc/ that calls getenv.
// One parser: a knob is unset or a decimal integer (strtoll: "" and text without leading digits read as 0).  A switch is "value != 0"; a mode
// knob is -1 (unset or negative: the launcher's own rule) or the forced value.  CACHED knobs are read once per process (a test that switches
// one starts a child process), LIVE knobs at every call (tests switch them within one process).  The derived predicates (og_mlp_fused_enabled,
// og_mlp_small_wanted, ...) stay beside their kernels and call these accessors; the q | k | v projection plan (og_proj_plan.h, plain C++ that a
// host-only program runs) takes the values of its knobs as plain ints from og_proj_knobs() (og_common.h).
#pragma once
#include <stdint.h>
#include <stdlib.h>

inline bool og_knob_parse(const char* name, long long* v) { const char* e = getenv(name); if (e) *v = strtoll(e, nullptr, 10); return e != nullptr; }
inline long long og_knob_value(const char* name, long long unset) { long long v; return og_knob_parse(name, &v) ? v : unset; }
#define OG_KNOB_CACHED(T, fn, name, unset) inline T fn() { static const T v = (T)og_knob_value(name, unset); return v; }
#define OG_KNOB_LIVE(T, fn, name, unset) inline T fn() { return (T)og_knob_value(name, unset); }

// ---- api.hip ----
OG_KNOB_CACHED(bool, og_knob_roctx, "OG_ROCTX", 0)                            // 1: every og_forward* call pushes / pops named roctx ranges
// ---- og_proj_plan.h (with OG_PROJ_STREAM, OG_GEMM_ROW_SPLIT, OG_GEMM_TILE, OG_GEMM_BIG2 below) ----
OG_KNOB_CACHED(int, og_knob_proj_small, "OG_PROJ_SMALL", -1)                  // 0 / 1 forces proj_small_kernel off / on (default: <= 8192 rows per launch)
// ---- gemm_f16x3.hip, gemm_f32.hip (experiments) ----
OG_KNOB_CACHED(int, og_knob_gemm_tile, "OG_GEMM_TILE", 0)                     // 128 / 256 forces the tile family
OG_KNOB_CACHED(bool, og_knob_gemm_big2, "OG_GEMM_BIG2", 1)                    // 0 = the first-generation 256-tile kernel
OG_KNOB_CACHED(bool, og_knob_gemm_row_split, "OG_GEMM_ROW_SPLIT", 1)          // 0 = a row-split GEMM as two launches
OG_KNOB_CACHED(bool, og_knob_gemm_fast_epi, "OG_GEMM_FAST_EPI", 1)            // 0 = the general epilogue for launches of whole tiles too
OG_KNOB_CACHED(bool, og_knob_gemm_spec_epi, "OG_GEMM_SPEC_EPI", 1)            // 0 = the epilogue arithmetic as a run-time mode everywhere
OG_KNOB_CACHED(int, og_knob_gemm_f32_bn, "OG_GEMM_F32_BN", 0)                 // 128 keeps 128-column tiles above N = 64
OG_KNOB_CACHED(int, og_knob_gemm_f32_bm, "OG_GEMM_F32_BM", 0)                 // 64 / 128 forces the rows per tile
OG_KNOB_CACHED(int64_t, og_knob_gemm_f32_short_below, "OG_GEMM_F32_SHORT_BELOW", 1024)   // 64-row tiles below this many workgroups
// ---- mlp_fused.hip ----
OG_KNOB_CACHED(bool, og_knob_mlp_fused, "OG_MLP_FUSED", 1)                    // experiments: 0 = fc.0 and fc.3 as two GEMM launches
OG_KNOB_CACHED(int, og_knob_mlp_small, "OG_MLP_SMALL", -1)                    // 0 / 1 forces mlp_small_kernel off / on (default: <= 8192 rows)
OG_KNOB_CACHED(bool, og_knob_proj_parts, "OG_PROJ_PARTS", 1)                  // 0 = proj_small_kernel with one workgroup per token tile
OG_KNOB_CACHED(int, og_knob_proj_stream, "OG_PROJ_STREAM", -1)                // 0 / 1 forces proj_stream_kernel off / on; 2 (experiment): batches, at K = 256 whole q | k | v launches only
// ---- attention.hip ----
OG_KNOB_CACHED(bool, og_knob_attn_dma, "OG_ATTN_DMA", 1)                      // 0 keeps the register-staged kernel at dh = 32 / 64 (A/B runs)
OG_KNOB_CACHED(int, og_knob_attn_ksplit, "OG_ATTN_KSPLIT", -1)                // 0 / 1 forces the key split over the halves of an 8-wave workgroup
OG_KNOB_CACHED(int, og_knob_attn_gsplit, "OG_ATTN_GSPLIT", -1)                // 0 / 2 / 4 forces the key tiles of a query tile onto 1 / 2 / 4 workgroups
OG_KNOB_CACHED(int, og_knob_attn_gs_maxwg, "OG_ATTN_GS_MAXWG", 0)             // experiments: the most workgroups a grid-split launch may have (> 0)
OG_KNOB_LIVE(bool, og_knob_attn_gs_scatter, "OG_ATTN_GS_SCATTER", 0)          // tests: 1 deals the parts of a grid-split tile to different XCDs
OG_KNOB_CACHED(int, og_knob_attn_p16, "OG_ATTN_P16", -1)                      // 1 = the 16x16x32 pipelined kernel (dh = 64)
OG_KNOB_CACHED(int, og_knob_attn_pipe, "OG_ATTN_PIPE", -1)                    // 1 = the software-pipelined tile loop; 2 = its eight-wave form (OG_ATTN_PIPE8 builds)
// experiments (scripts/bench_attention.py), LIVE: when set, og_attention's `vl` holds the 8-bit rows of the MX form and the value is their scale exponent
inline bool og_knob_attn_mx_sv(int* sv) { long long v = 0; const bool set = og_knob_parse("OG_ATTN_MX_SV", &v); *sv = (int)v; return set; }
// ---- sinkhorn.hip, sinkhorn_resident.hip, sinkhorn_train.hip ----
OG_KNOB_CACHED(bool, og_knob_sinkhorn_robust, "OG_SINKHORN_ROBUST", 0)        // experiments: 1 = max-subtracted streaming iterations only
OG_KNOB_LIVE(int, og_knob_sinkhorn_resident, "OG_SINKHORN_RESIDENT", 1)       // 0: streaming kernels only; 1: on-chip-resident iterations when the batch is co-resident and big enough to pay off; 2: whenever it is co-resident (tests)
OG_KNOB_LIVE(int, og_knob_sinkhorn_few, "OG_SINKHORN_FEW", -1)                // resident few-pairs geometry: 0 = never, 4 / 8 = that geometry when it exists, 1 = the finest
OG_KNOB_LIVE(bool, og_knob_sinkhorn_force_timeout, "OG_SINKHORN_FORCE_TIMEOUT", 0)   // tests: 1 = behave as if a peer workgroup of the resident schedule never arrived
OG_KNOB_LIVE(bool, og_knob_sinkhorn_agent_scope, "OG_SINKHORN_AGENT_SCOPE", 0)       // experiments / tests: 1 = the resident kernel never takes its XCD-local path
OG_KNOB_LIVE(int, og_knob_sk_fast_rows, "OG_SK_FAST_ROWS", 0)                 // experiments: 32 / 64 / 128 rows per workgroup of the dual-stabilised sweep
inline int og_knob_sk_fast_nt() { long long v; return og_knob_parse("OG_SK_FAST_NT", &v) ? (v != 0) : -1; }   // experiments, LIVE: 0 / 1 forces plain / non-temporal loads there; -1: unset
OG_KNOB_CACHED(int, og_knob_sk_bwd_rows_grid, "OG_SK_BWD_ROWS_GRID", 0)       // experiments: row workgroups of the backward sweeps (> 0; default 128)
#undef OG_KNOB_CACHED
#undef OG_KNOB_LIVE
