/*
 * openglue_amd.h -- C ABI of the MI355X (gfx950) SuperGlue hot path.
 *
 * Drop-in boundary for ucuapps/OpenGlue's keypoint-graph matcher.  The reference has no FFI or
 * operator registry: its plugin point is the Python class
 *     models/superglue/superglue.py:11   class SuperGlue(nn.Module)
 *     models/superglue/superglue.py:29   def forward(self, data) -> dict
 * constructed at models/matching_module.py:44 and inference.py:74, and the match extraction that
 * consumes its `scores` at models/matching_module.py:174-187 / inference.py:176-190.
 * openglue_amd/superglue.py keeps that Python signature and calls the functions below through
 * ctypes; any other host (C, C++, a cgo/JNI stub) can bind the same symbols.
 *
 * Conventions
 *   - plain C types only; no torch / HIP types in signatures (the stream is passed as void*,
 *     i.e. a hipStream_t; NULL = the default stream).
 *   - the library never allocates or frees device memory and keeps no global state: inputs,
 *     packed weights, workspace and outputs are caller-owned device buffers (fp32 unless noted).
 *   - every function only ENQUEUES work on `stream` (no internal synchronisation), so it composes
 *     with the caller's stream/allocator semantics and can be captured into a hipGraph.
 *   - return value: 0 = success; negative = OG_E_* invalid argument; positive = hipError_t of a
 *     failed launch.  Nothing throws across the ABI.
 *   - layouts are token-major: a set of n keypoints with C channels is an [n][C] row-major matrix.
 */
#ifndef OPENGLUE_AMD_H
#define OPENGLUE_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OG_ABI_VERSION 14

#define OG_E_INVALID   (-1)  /* NULL pointer / non-positive size                         */
#define OG_E_SHAPE     (-2)  /* unsupported shape (see og_check_shape)                   */
#define OG_E_ALIGN     (-3)  /* a device pointer is not 16-byte aligned                  */
#define OG_E_FLAG      (-4)  /* unknown flag bits                                        */
#define OG_E_RANGE     (-5)  /* og_pack_weights: a folded weight is not finite (or beyond 2^40).  Large finite weights -- e.g. a BatchNorm
                                fold over a dead channel with running_var ~ 0 -- are packed with a smaller per-matrix pre-scale   */

/* config flags (reference keys: superglue.py:18-19 `residual`, `no_descriptors`;
 * attention_gnn.py:51-52 `use_offset`) */
#define OG_FLAG_RESIDUAL        1
#define OG_FLAG_USE_OFFSET      2
#define OG_FLAG_NO_DESCRIPTORS  4
#define OG_FLAG_LINEAR_ATTENTION 16  /* attention_gnn.attention = 'linear': elu+1 linear attention (attention.py:22-40) instead of softmax */
#define OG_FLAG_FAVOR_RELU      32  /* attention_gnn.attention = 'favor_relu': generalised FAVOR+ attention with ReLU random features
                                       (attention.py:43-95, __init__.py:19-25): phi(x) = relu(P x d^-1/4) + 1e-8 on q and k, P the
                                       [2D][D] buffer og_layer_params.favor_projection, then linear attention over the 2D features.
                                       As in the reference this needs num_heads == 1 (its matmul of P with the per-head tensors only
                                       type-checks when the head size equals D); D <= 256.  Not combinable with LINEAR_ATTENTION. */
#define OG_FLAG_SIREN_ENCODER   8   /* positional_encoding.encoder_name = FeedForwardNetSiren: [Conv, sin(30x)]*h + Conv,
                                       no BatchNorm (models/utils.py:23-45); og_params.enc_bn is ignored */

#define OG_MAX_HIDDEN 8

/* Everything SuperGlue.__init__ reads from its config (superglue.py:16-27, 64, 108-109) plus the
 * batch geometry of one call.  Within one call every pair has m keypoints in image 0 and n in
 * image 1 (m != n allowed), as the reference requires. */
typedef struct og_shape {
    int32_t batch;                  /* B image pairs                                             */
    int32_t m, n;                   /* keypoints per image 0 / image 1                           */
    int32_t desc_dim;               /* D = descriptor_dim = attention_gnn.embed_dim (mult. of 64) */
    int32_t num_heads;              /* H; head h owns channels h*D/H .. (h+1)*D/H-1 (attention_gnn.py:24-26); D/H in {16,32,64,128} (128, round 6: register-staged attention kernel; training backward GEMM by GEMM)
                                       (OG_FLAG_LINEAR_ATTENTION: D/H in {16,32,64} only, 128 is OG_E_SHAPE; OG_FLAG_FAVOR_RELU: H == 1, any D <= 256) */
    int32_t num_stages;             /* L self+cross stages (attention_gnn.py:84-89)              */
    int32_t side_info;              /* s = positional_encoding.side_info_size (2+s <= 32)        */
    int32_t num_hidden;             /* len(positional_encoding.hidden_layers_sizes) <= OG_MAX_HIDDEN */
    int32_t hidden[OG_MAX_HIDDEN];  /* e.g. 32, 64, 128 (config/config.yaml:45)                  */
    int32_t sinkhorn_iters;         /* otp.num_iters                                             */
    float   sinkhorn_reg;           /* otp.reg                                                   */
    int32_t flags;                  /* OG_FLAG_*                                                 */
    float   match_threshold;        /* inference.match_threshold (config/config.yaml:40)         */
} og_shape;

/* ---- host-side parameter views (fp32, HOST memory), names as in the reference state-dict ---- */
typedef struct og_conv {            /* nn.Conv1d(kernel_size=1): weight [out][in] row-major, bias [out] */
    const float* weight;
    const float* bias;
} og_conv;

typedef struct og_bn {              /* nn.BatchNorm1d, eval mode (running statistics), eps = 1e-5 */
    const float* weight;
    const float* bias;
    const float* running_mean;
    const float* running_var;
} og_bn;

typedef struct og_layer_params {    /* attention_gnn.layers.{l}.module.*  (attention_gnn.py:35-41, 9-20) */
    og_conv in_proj_q, in_proj_k, in_proj_v, out_proj;   /* mha.*  [D][D]          */
    og_conv fc0;                                         /* fc.0   [2D][2D]        */
    og_bn   fc_bn;                                       /* fc.2   BatchNorm1d(2D) */
    og_conv fc3;                                         /* fc.3   [D][2D]         */
    const float* favor_projection;                       /* mha.attention_func.projection_matrix [2D][D] (attention.py:53); read with
                                                            OG_FLAG_FAVOR_RELU only, may be NULL otherwise (ABI v4)                  */
} og_layer_params;

typedef struct og_params {
    og_conv enc_conv[OG_MAX_HIDDEN + 1];  /* positional_encoding.encoder.{0,3,6,..}            */
    og_bn   enc_bn[OG_MAX_HIDDEN];        /* positional_encoding.encoder.{2,5,8,..}            */
    const og_layer_params* layers;        /* 2*L entries: even = self, odd = cross             */
    og_conv linear_proj;                  /* linear_proj [D][D]                  (superglue.py:22) */
    const float* mix_coefs;               /* [D] (state-dict [D,1]); may be NULL without OG_FLAG_RESIDUAL (superglue.py:21) */
    float dustbin_score;                  /* dustbin_score                       (superglue.py:23) */
} og_params;

/* ---- device-side call arguments ---- */
typedef struct og_inputs {
    const float* keypoints0;          /* [B][m][2] pixel xy                   data['keypoints0']         */
    const float* keypoints1;          /* [B][n][2]                                                       */
    const float* descriptors0;        /* [B][m][D]                            data['local_descriptors0'] */
    const float* descriptors1;        /* [B][n][D]                                                       */
    const float* side_info0;          /* [B][m][s]                            data['side_info0']         */
    const float* side_info1;          /* [B][n][s]                                                       */
    float image0_wh[2];               /* (W, H) of image 0   (superglue.py:35-38, 74-78)                 */
    float image1_wh[2];
} og_inputs;

typedef struct og_outputs {
    float*   scores;                  /* [B][m+1][n+1] log-assignment incl. dustbins   'scores'          */
    float*   context_descriptors0;    /* [B][D][m] channel-first, as the reference returns them; may be NULL */
    float*   context_descriptors1;    /* [B][D][n]; may be NULL                                          */
    int64_t* matches0;                /* [B][m]  index into image 1 or -1 (matching_module.py:181); may be NULL */
    float*   matching_scores0;        /* [B][m]  exp(max) if mutual else 0;  NULL iff matches0 is NULL   */
    int64_t* matches1;                /* [B][n]  inference.py:188; may be NULL                           */
    float*   matching_scores1;        /* [B][n]; NULL iff matches1 is NULL                               */
} og_outputs;

int og_abi_version(void);

/* 0 if the shape is supported by this build, else OG_E_SHAPE / OG_E_FLAG. */
int og_check_shape(const og_shape* shape);

/* Size in bytes of the packed-weight blob / of the per-call workspace for `shape` (0 on error).
 * The packed size does not depend on batch, m, n. */
size_t og_packed_weights_bytes(const og_shape* shape);
size_t og_workspace_bytes(const og_shape* shape);

/* Host-side, one-off (re-run when parameters change): fold eval-mode BatchNorm into the following
 * conv (the reference order is Conv -> ReLU -> BN, models/utils.py:52-56), fold out_proj into fc.0,
 * concatenate and pre-scale the q/k/v projections, zero-pad the encoder MLP to MFMA tile sizes.
 * `packed_host` (og_packed_weights_bytes bytes, host memory) is then copied to the device by the
 * caller.  Arithmetic in double precision. */
int og_pack_weights(const og_shape* shape, const og_params* params, void* packed_host);

/* Introspection of the packed blob (offsets in floats).  All matrices are [out][in] row-major; the
 * GNN matrices are stored as split-f16 hl32 rows of 256 * w (see og_split_f16_hl / og_gemm_nt_f16x3 below:
 * [out][2*in] halves = out*in floats), everything else as fp32.
 *   enc_w[i] [enc_out[i]][enc_k[i]], enc_b[i] [enc_out[i]]   keypoint-encoder conv i, zero-padded (k: 32 | out: mult. of 64),
 *                                                            BatchNorm i-1 folded in
 *   layer l at layer0 + l*layer_stride:  wqkv [3D][D] (q rows pre-scaled by (D/H)^-1/2 * log2 e), bqkv [3D],
 *                                        w0 [2D][2D] = [W0a | Wm*Wo], b0 [2D], w3 [D][2D] (BN folded), b3 [D]
 *   wp [D][D] (hl32 rows of 256 * w like the GNN matrices), bp [D], alpha [D] = sigmoid(mix_coefs), dustbin [1] */
typedef struct og_packed_layout_t {
    int32_t n_enc;
    int32_t enc_k[OG_MAX_HIDDEN + 1], enc_out[OG_MAX_HIDDEN + 1];
    int64_t enc_w[OG_MAX_HIDDEN + 1], enc_b[OG_MAX_HIDDEN + 1];
    int64_t layer0, layer_stride, o_wqkv, o_bqkv, o_w0, o_b0, o_w3, o_b3;   /* o_w*: hl32 rows of 2K halves */
    int64_t wp, bp, alpha, dustbin, total;
    int64_t o_scale;  /* ABI v5: per layer, 4 floats {1 / S_qkv, 1 / S_0, 1 / S_3, 0}: every split-f16 matrix is stored as (hi, lo) halves of
                         S * w with its own power-of-two S = 256 unless 256 * max|w| would leave binary16 (a BatchNorm fold over a dead
                         channel, a huge gamma / sigma); the kernels multiply the accumulator by the stored 1 / S                    */
    int64_t scales;   /* ABI v5: 2 floats {1 / S_wp, 1 / S of the last encoder conv}                                                 */
    int64_t o_wmlp;   /* ABI v5: per layer, the SAME folded w0 / w3 once more as the fragment-major stream og_mlp_block consumes
                         (og_mlp_block_stream_bytes(D) bytes; -1 when D has no fused message-MLP kernel)                         */
    int64_t o_wqkvs;  /* ABI v7: per layer, the q | k | v matrix once more as the fragment-major stream og_proj_block consumes (the
                         small-batch projection kernel; N K 4 bytes; -1: D not 256 / 128, or favor_relu)   */
    int64_t o_wqkvb;  /* ABI v8: ... and a third time as the stream of the BATCH projection kernel (proj_stream_kernel: launches of more than
                         8192 token rows; N K 4 bytes; -1 as above).  og_proj_block_stream_bytes(N, K) = both streams, the small one first  */
} og_packed_layout_t;
int og_packed_layout(const og_shape* shape, og_packed_layout_t* layout);

/* The whole hot path: keypoint encoder -> L x (self, cross) attention -> final projection ->
 * score matrix -> log-domain Sinkhorn with dustbins -> scores (+ optional mutual-NN matches).
 * Replaces SuperGlue.forward (superglue.py:29-72) and, when outputs->matches0 != NULL, the match
 * extraction of matching_module.py:174-187 / inference.py:176-190. */
int og_forward(const og_shape* shape, const og_inputs* in, const void* packed_dev,
               void* workspace_dev, const og_outputs* out, void* stream);

/* og_forward plus a copy of the RESIDUAL STREAM at one stage boundary, for per-stage parity tests (the reference's sub-modules:
 * positional_encoding.py:16-19 + superglue.py:52-55 for tap 0; attention_gnn.py:57-77, one DescriptorsSelfAttention /
 * DescriptorsCrossAttention = ResidualAttentionMessagePropagation on both images, for tap k >= 1):
 *   tap = 0:        x = local_descriptors + keypoint_encoder(...) as it enters the GNN;
 *   tap = k in 1..2L: x after GNN layer k - 1 (even layers self, odd layers cross);
 * tap_x: [B*m + B*n][D] fp32, token-major, image-0 sets first (what the kernels hold as (hi, lo) f16 pairs, merged).
 * Everything else as og_forward (the call runs the whole path). */
int og_forward_tap(const og_shape* shape, const og_inputs* in, const void* packed_dev, void* workspace_dev,
                   const og_outputs* out, void* stream, int32_t tap, float* tap_x);

/* Per-stage entries SURVEY.md 8(b) names beside og_sinkhorn / og_attention / og_mlp_block / og_extract_matches:
 * og_keypoint_encoder -- superglue.py:44-55 with positional_encoding.py:16-19 and the normalisation of :74-78: x = local_descriptors +
 *   encoder(normalised keypoints, side info) for all B*m + B*n tokens (image-0 sets first), fp32 [T][D] -- exactly what og_forward_tap(tap = 0)
 *   copies out, without running the rest of the path (outputs: none but x_out; workspace and packed weights as og_forward).
 * og_scores -- superglue.py:64, 80-86: S[b] = g0[b] g1[b]^T * D^-1/2 for token-major fp32 descriptors g0 [B][m][D], g1 [B][n][D] into
 *   S [B][m][lds] (lds >= n, multiple of 4), exact fp32 MFMA (og_gemm_nt).  og_forward forms the same product from the (hi, lo) rows its
 *   final projection leaves, on the split-f16 kernel. */
int og_keypoint_encoder(const og_shape* shape, const og_inputs* in, const void* packed_dev, void* workspace_dev, float* x_out, void* stream);
int og_scores(const float* g0, const float* g1, int32_t batch, int32_t m, int32_t n, int32_t D, float* S, int64_t lds, void* stream);

/* Ragged batch (BASELINE config 5): pair b has lens0[b] keypoints in image 0 and lens1[b] in image 1
 * (host arrays, batch <= OG_MAX_RAGGED; shape->m / shape->n are the maxima).  Every tensor is PACKED without
 * padding in pair order: keypoints0 [sum m_b][2], descriptors0 [sum m_b][D], ..., scores = the
 * [m_b+1][n_b+1] blocks one after the other, matches0 / matching_scores0 [sum m_b], matches1 [sum n_b],
 * context_descriptors0 = the channel-first [D][m_b] blocks one after the other (may be NULL), likewise 1.
 * image0_wh / image1_wh: host arrays [batch][2] = (W, H) of every pair's images (keypoint normalisation,
 * superglue.py:35-41, 74-78); NULL = in->image{0,1}_wh for all pairs.
 * The result of pair b equals og_forward on that pair alone (the reference has no masks: SURVEY.md 3.5). */
#define OG_MAX_RAGGED 64
int og_forward_ragged(const og_shape* shape, const int32_t* lens0, const int32_t* lens1, const float* image0_wh,
                      const float* image1_wh, const og_inputs* in, const void* packed_dev, void* workspace_dev,
                      const og_outputs* out, void* stream);

/* Profiling variant of og_forward (bench.py): same work, but every launch group is bracketed by HIP
 * events recorded on `stream`; the call SYNCHRONISES the stream and returns the summed elapsed
 * milliseconds and the number of bracketed launch groups per kernel class.  GEMM and attention are
 * bracketed per kernel launch, Sinkhorn / matches per stage (many small launches: og_sinkhorn_schedule tells which). */
#define OG_STAGE_ENCODER_INPUT 0
#define OG_STAGE_GEMM          1
#define OG_STAGE_ATTENTION     2
#define OG_STAGE_SINKHORN      3
#define OG_STAGE_MATCHES       4
#define OG_STAGE_GEMM_F16X3    5   /* split-f16 GEMMs (q/k/v projections, final projection, score matrix, last encoder conv; the message
                                      MLP as two launches when it is not fused); OG_STAGE_GEMM = the exact-fp32 ones */
#define OG_STAGE_MLP_FUSED     6   /* ABI v5: the fused message-MLP kernel (csrc/mlp_fused.hip), one launch per bracket */
#define OG_NUM_STAGES          7
int og_forward_profiled(const og_shape* shape, const og_inputs* in, const void* packed_dev,
                        void* workspace_dev, const og_outputs* out, void* stream,
                        float* stage_ms /*[OG_NUM_STAGES]*/, int32_t* stage_launches /*[OG_NUM_STAGES]*/);
int og_forward_ragged_profiled(const og_shape* shape, const int32_t* lens0, const int32_t* lens1, const float* image0_wh,
                               const float* image1_wh, const og_inputs* in, const void* packed_dev, void* workspace_dev,
                               const og_outputs* out, void* stream, float* stage_ms, int32_t* stage_launches);

/* ---- per-stage entry points (unit parity tests; also usable on their own) ---- */

/* C[z] = epilogue(A[z] * B[z]^T): A [M][K] (lda), B [N][K] (ldb), exact fp32 MFMA.
 * v = acc + bias[col]; relu; if res: alpha ? alpha[col]*v + (1-alpha[col])*res : v + res; v *= scale. */
int og_gemm_nt(const float* A, int64_t lda, int64_t strideA, const float* B, int64_t ldb, int64_t strideB,
               float* C, int64_t ldc, int64_t strideC, int32_t M, int32_t N, int32_t K, int32_t batch,
               const float* bias, int32_t relu, const float* res, int64_t ldr, const float* alpha,
               float scale, void* stream);

/* The same kernel with K-MAJOR operands (exact fp32 MFMA, no epilogue but `scale`): B[z] is stored [K][N] (row stride ldb) and, with
 * a_kmajor, A[z] is stored [K][M] -- the layouts the backward products of a 1x1 conv and of attention come in (dX = dZ W with
 * W [out][in]; dW = dZ^T X with both operands [tokens][channels]), so that no transposed copy of a token-sized tensor is made.
 * k_total > 0 (a_kmajor only) = split-K: problem z contracts k-rows [z K, min((z+1) K, k_total)) -- strideA = K*lda, strideB = K*ldb
 * cut one long contraction into `batch` partial products C[z] the caller sums.  a_colsum (a_kmajor only, ldc > N): column N of C[z]
 * receives sum_k A[k][m] -- the bias gradient of the conv comes out of the weight-gradient launch.  lda, ldb multiples of 4;
 * K % 4 == 0 only when A is K-contiguous (a_kmajor == 0). */
int og_gemm_kmajor(const float* A, int64_t lda, int64_t strideA, int32_t a_kmajor, const float* B, int64_t ldb, int64_t strideB,
                   float* C, int64_t ldc, int64_t strideC, int32_t M, int32_t N, int32_t K, int32_t batch, int32_t k_total,
                   int32_t a_colsum, float scale, void* stream);

/* Split-f16 representation used inside the GNN: x = hi + lo with hi = f16(x), lo = f16(x - hi), both IEEE
 * binary16 (|x| < 65504; lo may be subnormal, the matrix cores honour it), stored either as two planes or in the "hl32" row format the GEMM consumes: one row of
 * 2K halves per token, hi and lo interleaved in groups of 32 channels
 * [hi 0..31 | lo 0..31 | hi 32..63 | lo 32..63 | ...] so that a 32-channel k-slab is one 128-byte line.
 * og_split_f16 converts n (multiple of 4) fp32 values into two planes; og_split_f16_hl converts
 * x [rows][cols] (row stride ldx, cols % 32 == 0) into hl32 rows (row stride ldo >= 2*cols halves). */
int og_split_f16(const float* x, int64_t n, void* hi, void* lo, void* stream);
int og_split_f16_hl(const float* x, int64_t rows, int32_t cols, int64_t ldx, void* out, int64_t ldo, void* stream);

/* C = epilogue(A * B^T) with A [M][K], B [N][K] in the hl32 row format (lda, ldb: row strides in halves,
 * multiples of 8, >= 2K; K % 32 == 0): 3 f16 MFMAs per product, fp32 accumulate, fp32-class accuracy.
 * v = acc * scale + bias[col] (scale undoes a power-of-two pre-scale of B: og_pack_weights stores 256 * W so
 * that the lo parts of small weights stay normal numbers); relu; + res[row][col] (fp32, ldr); written as fp32 (C32, may be NULL) and/or in
 * split-f16 form: c_hl == 0 -> two planes Ch/Cl with leading dimension ldch; c_hl != 0 -> hl32 rows at Ch
 * (row stride ldch halves, Cl ignored, N % 32 == 0).  N % 4 == 0. */
int og_gemm_nt_f16x3(const void* A, int64_t lda, const void* B, int64_t ldb, int32_t M, int32_t N, int32_t K,
                     float scale, const float* bias, int32_t relu, const float* res, int64_t ldr, float* C32, int64_t ldc,
                     void* Ch, void* Cl, int64_t ldch, int32_t c_hl, void* stream);
/* The same with the residual given as hl32 rows (res_hl, row stride ldrh halves; may alias Ch when c_hl != 0: every element is read
 * before it is written by the same lane): v += hi + lo.  This is the form of the GNN's fc.3 (attention_gnn.py:55: desc_q + fc(message)):
 * og_forward keeps the residual stream as (hi, lo) rows.  C32 may be NULL when a split-f16 output is given. */
int og_gemm_nt_f16x3_reshl(const void* A, int64_t lda, const void* B, int64_t ldb, int32_t M, int32_t N, int32_t K,
                           float scale, const float* bias, int32_t relu, const void* res_hl, int64_t ldrh, float* C32, int64_t ldc,
                           void* Ch, void* Cl, int64_t ldch, int32_t c_hl, void* stream);

/* The message MLP of one GNN layer (attention_gnn.py:53-55 with models/utils.py:48-58, BatchNorm and out_proj folded as
 * og_pack_weights does) as ONE launch, in place on M token rows of hl32 rows [x | O] (4D halves used per row, row stride ld halves):
 *     x <- x + W3 relu(W0 [x ; O] + b0) + b3,     W0 [2D][2D], W3 [D][2D] row-major fp32, b0 [2D], b3 [D] (device).
 * The hidden activation lives in registers (csrc/mlp_fused.hip); the weights are consumed as a fragment-major stream of (hi, lo)
 * halves of 256 w that og_mlp_block_pack writes on the host (og_mlp_block_stream_bytes(D) bytes, 0 = D not supported: D == 256, and since
 * ABI v8 D == 128, the reference's SIFT / HardNet descriptor width).
 * Same arithmetic as og_gemm_nt_f16x3 (relu) followed by og_gemm_nt_f16x3_reshl. */
/* ABI v7.  A 1x1 conv of the residual stream for FEW token rows (the q / k / v projections of attention_gnn.py:43-47 when one or a few
 * image pairs are matched: og_forward uses it for launches of <= 8192 rows): y[M][N] = x W^T + bias on the x halves of M hl32 rows
 * (the first 2K halves of a row, row stride ld halves), W [N][K] row-major fp32, K = 256 or (ABI v8) 128, N a multiple of 32; the result leaves as
 * (hi, lo) f16 planes yh / yl [M][ldy].  32-token workgroups whose 8 waves split the output blocks (csrc/mlp_fused.hip:
 * proj_small_kernel); the weights are consumed as a fragment-major stream of (hi, lo) halves of 256 w that og_proj_block_pack writes on
 * the host (og_proj_block_stream_bytes(N, K) bytes, 0 = shape not supported).  Rows below split_row get the output columns
 * [32 a0, 32 a1), the others [32 b0, 32 b1) (split_row a multiple of 32, or 0 / >= M for one range).  inv_scale_dev: DEVICE float,
 * 1 / 256 for streams packed here.  Same arithmetic as og_gemm_nt_f16x3.  ABI v8: og_proj_block takes K; launches of more than 8192 rows whose column
 * ranges are whole groups of 128 channels (and split_row a multiple of 128, yh / yl 128-byte aligned) take the batch kernel (proj_stream_kernel:
 * 128-token workgroups, the x fragments in registers, weights through an LDS ring) -- og_proj_block_pack writes its stream behind the small-batch
 * one.  OG_PROJ_STREAM=0 / 1 forces either kernel.  ABI v10: N (the row count of W the stream was packed for) is an argument -- it locates the batch
 * stream behind the small-batch one; before, it was read off ldy, which silently mis-addressed the stream for an output plane padded beyond N.
 * ldy >= N, a multiple of 64 halves for the batch kernel.  At K = 256, launches of more than 8192 rows whose planes are exactly as wide as the matrix
 * (ldy == N, og_forward's own geometry), whose column ranges are whole 256-column slabs (a0 .. b1 multiples of 8) and whose split_row is a multiple
 * of 32 take the weight-stationary kernel og_forward runs for 256-d batches (csrc/proj_wstat.hip: proj_wstat_kernel; it reads the small-batch
 * stream, nothing more is packed); OG_PROJ_STREAM = 0 / 1 keeps such a launch on the kernels above. */
size_t og_proj_block_stream_bytes(int32_t N, int32_t K);
int og_proj_block_pack(int32_t N, int32_t K, const float* W, void* stream_host);
int og_proj_block(const void* x_rows, int64_t ld, int32_t M, int32_t K, int32_t N, const void* stream_dev, const float* bias, const float* inv_scale_dev,
                  void* yh, void* yl, int64_t ldy, int32_t split_row, int32_t a0, int32_t a1, int32_t b0, int32_t b1, void* stream);

size_t og_mlp_block_stream_bytes(int32_t D);
int og_mlp_block_pack(int32_t D, const float* W0, const float* W3, void* stream_host);
int og_mlp_block(int32_t D, void* xo_rows, int64_t ld, int32_t M, const void* stream_dev, const float* b0, const float* b3,
                 void* stream);

/* softmax attention (attention.py:8-19) for `batch` independent problems and H heads, operands and
 * result as split-f16 planes: q [batch][nq][ldq] (columns h*dh.. of row i = head h, PRE-SCALED by
 * dh^-0.5 * log2(e): the kernel evaluates softmax as 2^(q.k - max)), k, v [batch][nk][ld*],
 * out [batch][nq][ldo]; leading dimensions in elements.  dh in {16,32,64,128}.
 * ABI v6: lse (may be NULL) [batch][num_heads][nq] receives the row log-sum-exp of the scaled scores in natural units,
 * ln sum_j exp(dh^-0.5 q_i . k_j) -- what a backward pass that recomputes the attention matrix needs (og_attention_backward). */
int og_attention(const void* qh, const void* ql, int64_t ldq, const void* kh, const void* kl, int64_t ldk,
                 const void* vh, const void* vl, int64_t ldv, void* oh, void* ol, int64_t ldo, int32_t batch,
                 int32_t nq, int32_t nk, int32_t num_heads, int32_t dh, float* lse, void* stream);

/* log-domain Sinkhorn with implicit dustbins (superglue.py:88-111 + optimal_transport.py:20-28):
 * S [B][m][lds] (lds % 4 == 0) is the raw score matrix, `dustbin` the learnt bin score; writes
 * scores [B][m+1][n+1] = S_aug/reg + u + v - norm.  workspace: og_sinkhorn_workspace_bytes. */
size_t og_sinkhorn_workspace_bytes(int32_t batch, int32_t m, int32_t n);
int og_sinkhorn(const float* S, int64_t lds, float dustbin, int32_t batch, int32_t m, int32_t n,
                int32_t iters, float reg, float* scores, void* workspace_dev, void* stream);

/* Diagnostics: state of the last og_sinkhorn / og_forward Sinkhorn stage that ran on this workspace.  Copies two words on a private stream
 * after the work ALREADY ENQUEUED ON THE NULL STREAM has finished (an event, no device-wide synchronisation: other streams keep running and
 * are not waited for -- a caller that launched on its own stream synchronises that stream first, as openglue_amd/superglue.py does).
 * State of the last og_sinkhorn / og_forward Sinkhorn stage that ran on
 * this Sinkhorn workspace (every call resets it).
 *   0 = completed normally (streaming kernels, or the on-chip-resident kernel without incident);
 *   2 = a cross-workgroup wait of the on-chip-resident iteration kernel timed out (the workgroups of a launch must be
 *       co-resident; the launcher checks that against the CU count, but another stream or process holding CUs can still break it)
 *       and the safety-net kernel enqueued behind it solved the problem again, one workgroup per pair: the scores are VALID, the
 *       call was slow (milliseconds);
 *   3 = a NON-FINITE value was written to the scores: something upstream overflowed or was NaN -- an activation beyond the binary16
 *       range of the split-f16 operands (|x| >= 65504), non-finite inputs.  The scores are invalid;
 *   1 = timed out and not recomputed (cannot happen with this build's launch sequence; scores invalid); -1 = bad arguments.
 * For n <= 4096 and at least 2^18 matrix entries per call (OG_SINKHORN_RESIDENT=0 disables, =2 drops the size threshold) iterations
 * 2..iters run with the plan matrices held in registers + LDS, one launch per round of co-resident pairs (csrc/sinkhorn_resident.hip).
 * OG_SINKHORN_FORCE_TIMEOUT=1 (tests) makes those launches behave as if they had timed out. */
int og_sinkhorn_status(const void* sinkhorn_workspace_dev, int32_t batch, int32_t m, int32_t n);
/* Which schedule og_sinkhorn / og_forward take for a UNIFORM batch of this shape in this process (environment switches and the
 * device's CU count included): k >= 1 = first iteration streaming, then k launches of the on-chip-resident kernel for iterations
 * 2..iters (one per round of co-resident pairs: 32 pairs of 1024 x 1024, 8 of 2048 x 2048, 2 of 4096 x 4096 on 256 CUs) + the
 * safety-net and scores kernels; 0 = streaming (2 launches per iteration + 1).  bench.py uses it to name what its Sinkhorn bracket
 * timed.  og_sinkhorn_schedule_ragged: the same for a ragged batch (host arrays of per-pair sizes, batch <= OG_MAX_RAGGED): pairs are
 * grouped by width class and packed one pair per XCD slot range; 0 when any pair has no resident geometry. */
int og_sinkhorn_schedule(int32_t batch, int32_t m, int32_t n, int32_t iters);
int og_sinkhorn_schedule_ragged(int32_t batch, const int32_t* lens0, const int32_t* lens1, int32_t iters);
/* How the on-chip-resident schedule tiles ONE pair of m x n keypoints on a part with 8 XCDs x 32 CUs (host arithmetic only, no device):
 * out4 = {W, X, Gx, pairs per launch} -- workgroup tiles of (128 / W) rows x (1024 W) columns, X column blocks (one per XCD) x Gx row blocks;
 * returns 0, or OG_E_SHAPE when the shape has no resident geometry (more than 4096 rows or columns: streaming kernels). */
int og_sinkhorn_resident_geometry(int32_t m, int32_t n, int32_t* out4);
/* Host arithmetic only (8 XCDs x 32 CUs assumed): the row slots per WAVE a uniform launch of `batch` pairs takes in the resident kernel: 16 (workgroup
 * tiles of 128 / W rows), or -- launches of few pairs of <= 1024 x 1024 keypoints, the reference's one-pair-per-call regime (inference.py:214-235) --
 * 4 (a pair = 32 tiles of 32 x 1024: up to 8 pairs) or 8 (16 tiles of 64 x 1024: 9 to 16 pairs); 0 = no resident geometry.  OG_SINKHORN_FEW=0 / 1 / 4 / 8
 * overrides. */
int og_sinkhorn_resident_rows_per_wave(int32_t batch, int32_t m, int32_t n);
/* Host arithmetic only (8 XCDs x 32 CUs assumed): the resident launches a RAGGED batch of per-pair sizes takes and the bytes of the
 * resident exchange slot the widest of them touches, out2 = {launches, bytes}; OG_E_SHAPE when some pair has no one-XCD geometry (the
 * batch streams).  The slot og_sinkhorn_workspace_bytes(batch, max m, max n) reserves is sized for the widest tile class any pair with
 * n_b <= max n can take, so `bytes` always fits it (tests/test_boundary_cpu.py checks that over random plans). */
int og_sinkhorn_resident_ragged_footprint(int32_t batch, const int32_t* lens0, const int32_t* lens1, int64_t* out2);
/* The same check for the workspace of an og_forward / og_forward_ragged call with this shape (for ragged calls: the shape
 * that was passed, i.e. the maxima).  Waits like og_sinkhorn_status (NULL stream only).  Return values as og_sinkhorn_status. */
int og_forward_status(const og_shape* shape, const void* workspace_dev);

/* ---- training slice of the optimal-transport layer (reference: autograd through superglue.py:88-111 +
 * optimal_transport.py:20-28, consumed by the NLL of utils/losses.py:7-53) ----
 * og_sinkhorn_train_forward: like og_sinkhorn (max-subtracted iterations only) but keeps the duals of every iteration in
 * the training workspace; og_sinkhorn_backward: given grad_scores = dL/dscores [B][m+1][n+1] it back-propagates through the
 * `iters` unrolled iterations and writes dS [B][m][ldds] (gradient w.r.t. the raw score matrix) and *d_dustbin (device
 * scalar, may be NULL; gradient w.r.t. dustbin_score).  n <= 4159, iters >= 1.  fp32 atomics: gradients reproducible to
 * rounding, not bit for bit.  The same workspace must be passed to both calls.  ABI v6: dustbin_dev (device scalar, or NULL =
 * use the host value `dustbin`) -- the learnable dustbin_score is read ON the device, the training step never waits for the GPU. */
size_t og_sinkhorn_train_workspace_bytes(int32_t batch, int32_t m, int32_t n, int32_t iters);
int og_sinkhorn_train_forward(const float* S, int64_t lds, float dustbin, const float* dustbin_dev, int32_t batch, int32_t m, int32_t n,
                              int32_t iters, float reg, float* scores, void* train_workspace_dev, void* stream);
int og_sinkhorn_backward(const float* S, int64_t lds, float dustbin, const float* dustbin_dev, int32_t batch, int32_t m, int32_t n, int32_t iters,
                         float reg, const float* grad_scores, void* train_workspace_dev, float* dS, int64_t ldds,
                         float* d_dustbin, void* stream);

/* ---- training slice: train-mode BatchNorm of the MLPs (reference models/utils.py:48-58, FeedForwardNet = Conv1d -> ReLU ->
 * nn.BatchNorm1d, in training mode: torch.nn.functional.batch_norm(training=True)) on TOKEN-MAJOR activations
 * x [rows][channels] (row stride ldx floats; the reference's [B, C, N] tensor with rows = B*N): batch statistics per channel
 * over all rows, y = (x - mean) / sqrt(biased var + eps) * weight + bias, running_mean / running_var updated in place with
 * `momentum` (running_var takes the unbiased variance), all like torch.  weight / bias / running_* / save_* may be NULL;
 * save_mean / save_invstd [channels] are what a backward pass needs.  channels % 4 == 0, ldx % 4 == 0, ldy % 4 == 0,
 * 16-byte aligned pointers; y may alias x.  workspace: og_batchnorm_train_workspace_bytes (0 = unsupported shape). */
size_t og_batchnorm_train_workspace_bytes(int64_t rows, int32_t channels);
int og_batchnorm_train_forward(const float* x, int64_t ldx, int64_t rows, int32_t channels, const float* weight,
                               const float* bias, float eps, float momentum, float* running_mean, float* running_var,
                               float* y, int64_t ldy, float* save_mean, float* save_invstd, void* workspace_dev,
                               void* stream);

/* Backward of the same block (autograd of relu + torch.nn.functional.batch_norm(training=True), i.e. of models/utils.py:53-55
 * during MatchingTrainingModule.training_step): a = the block's BatchNorm INPUT (the ReLU output), dy = dL/dy, save_mean /
 * save_invstd from the forward.  Writes dz = dL/d(pre-ReLU conv output) when relu_mask != 0 (else dL/da), dweight, dbias
 * (may be NULL).  Same shape rules and workspace size as the forward; dz may alias dy. */
int og_batchnorm_train_backward(const float* a, int64_t lda, const float* dy, int64_t lddy, int64_t rows, int32_t channels,
                                const float* weight, const float* save_mean, const float* save_invstd, int32_t relu_mask,
                                float* dz, int64_t lddz, float* dweight, float* dbias, void* workspace_dev, void* stream);
/* Helpers of the 1x1-conv backward on token-major activations (dW = dZ^T X as og_gemm_nt(dZ^T, X^T); db = column sums of dZ); kept
 * for callers of the NT form -- openglue_amd.train uses og_gemm_kmajor (operands as they lie, bias gradient in the same launch) since v6:
 * dst[c][r] = src[r][c]; out[c] = sum_r x[r][c] (workspace: og_batchnorm_train_workspace_bytes(rows, channels) is enough). */
int og_transpose_f32(const float* src, int64_t ld_src, int64_t rows, int32_t cols, float* dst, int64_t ld_dst, void* stream);
int og_colsum_f32(const float* x, int64_t ldx, int64_t rows, int32_t channels, float* out, void* workspace_dev, void* stream);

int og_transpose_f32_batched(const float* src, int64_t ld_src, int64_t stride_src, int64_t rows, int32_t cols, float* dst,
                             int64_t ld_dst, int64_t stride_dst, int32_t batch, void* stream);
/* Training-mode softmax attention keeps the attention matrix, like the reference (models/superglue/attention.py:8-19; autograd
 * needs it): og_softmax_rows turns S [rows][ld] (= scale * Q K^T from og_gemm_nt) into P in place, og_softmax_rows_backward turns
 * dP (= dO V^T) into dS = scale * P o (dP - rowsum(dP o P)) in place.  Columns [cols, ld) are zeroed. */
int og_softmax_rows(float* S, int64_t ld, int64_t rows, int32_t cols, void* stream);
int og_softmax_rows_backward(const float* P, float* dP, int64_t ld, int64_t rows, int32_t cols, float scale, void* stream);

/* Backward of multi-head softmax attention without the attention matrix (flash style, exact fp32 MFMA; csrc/attention_train.hip):
 * q, dout [batch][nq][D], k, v [batch][nk][D] token-major fp32, D = num_heads * dh, head h = columns [h dh, (h+1) dh), dh in {16, 32, 64}.
 * og_attention_train_lse: lse[batch][num_heads][nq] = log sum_j exp(scale q_i . k_j).
 * og_attention_backward: delta[batch][nq][num_heads] = sum_c dout o out over the head's columns (caller); writes dk, dv [batch][nk][D] and
 * og_attention_backward_parts(nk) partial dq tensors dq_part[part][batch][nq][D] (one per 64-key block; dq = their sum: deterministic,
 * no atomics). */
int og_attention_train_lse(const float* q, const float* k, int32_t batch, int32_t nq, int32_t nk, int32_t num_heads, int32_t dh,
                           float scale, float* lse, void* stream);
int og_attention_backward_parts(int32_t nk);
int og_attention_backward(const float* q, const float* k, const float* v, const float* dout, const float* lse, const float* delta,
                          int32_t batch, int32_t nq, int32_t nk, int32_t num_heads, int32_t dh, float scale, float* dq_part, float* dk,
                          float* dv, void* stream);
/* ABI v9 -- the same (the autograd of models/superglue/attention.py:8-19 inside attention_gnn.py:22-32) with ROW STRIDES (floats, multiples of 4, >= D) on q, k, v and on the dk, dv outputs, so that the training step hands over
 * column ranges of its [tokens][3D] projection matrix and receives dk, dv inside the [tokens][3D] gradient matrix (no slices copied out, no
 * concatenation); dout and dq_part rows stay D wide.  og_attention_delta: delta[row][h] = sum_c dout[row][h dh + c] out[row][h dh + c] for
 * contiguous [rows][num_heads * dh] tensors (what og_attention_backward wants as `delta`), one launch. */
int og_attention_backward_ld(const float* q, int64_t ldq, const float* k, int64_t ldk, const float* v, int64_t ldv, const float* dout,
                             const float* lse, const float* delta, int32_t batch, int32_t nq, int32_t nk, int32_t num_heads, int32_t dh,
                             float scale, float* dq_part, float* dk, int64_t lddk, float* dv, int64_t lddv, void* stream);
int og_attention_delta(const float* dout, const float* out, int64_t rows, int32_t num_heads, int32_t dh, float* delta, void* stream);
/* ABI v9 -- glue of the training step (MatchingTrainingModule.training_step, models/matching_module.py:93-105, through SuperGlue.forward) as single
 * launches (openglue_amd/train.py):
 * og_split_f16_rows: x [rows][cols] fp32 (row stride ldx) -> (hi, lo) binary16 planes (row stride ldo), columns [0, scale_cols) multiplied by
 *   s1, then s2, first (the q columns of a q | k | v matrix: dh^-1/2, then the log2(e) of og_attention's base-2 softmax);
 * og_merge_f16: out[i] = float(hi[i]) + float(lo[i]) (og_attention's output planes back to fp32);
 * og_splitk_reduce: the `parts` partial products part[p][rows][ld] of a split-K weight gradient (og_gemm_kmajor with batch = parts) summed in
 *   part order into dW [rows][cols]; db (may be NULL) [rows] = the sums of column `cols` (the a_colsum column: ld >= cols + 4 then). */
int og_split_f16_rows(const float* x, int64_t ldx, int64_t rows, int32_t cols, int32_t scale_cols, float s1, float s2, void* hi, void* lo,
                      int64_t ldo, void* stream);
int og_merge_f16(const void* hi, const void* lo, int64_t n, float* out, void* stream);
int og_splitk_reduce(const float* part, int32_t parts, int32_t rows, int64_t ld, int32_t cols, float* dW, float* db, void* stream);

/* mutual-NN match extraction from a scores tensor [B][m+1][n+1] (matching_module.py:174-187;
 * matches1/matching_scores1 as inference.py:183-188, may be NULL).  First maximal index wins.
 * workspace: og_matches_workspace_bytes. */
size_t og_matches_workspace_bytes(int32_t batch, int32_t m, int32_t n);
int og_extract_matches(const float* scores, int32_t batch, int32_t m, int32_t n, float match_threshold,
                       int64_t* matches0, float* matching_scores0, int64_t* matches1,
                       float* matching_scores1, void* workspace_dev, void* stream);

/* ---- the steps either side of the matcher in OpenGlue's inference loop ---- */

/* models/features/utils.py:54-65 prepare_features_output + models/laf_converter.py: lafs [tokens][2][3],
 * responses [tokens] -> keypoints [tokens][2] (LAF centre) and side_info [tokens][s].
 * method: 0 'none' (s=1), 1 'scale' (2), 2 'rotation' (3), 3 'scale_rotation' (4), 4 'affine' (6);
 * log_response: response -> log(response + 0.1).  LAF scale as kornia.feature.laf.get_laf_scale. */
int og_prepare_features(const float* lafs, const float* responses, int64_t tokens, int32_t method, int32_t log_response,
                        float* keypoints, float* side_info, void* stream);

/* inference.py:192-209: order-preserving compaction of the valid matches of a batch.
 * matches0 / matching_scores0 [B][m]; lafs0 [B][m][2][3], lafs1 [B][n][2][3] (both may be NULL).
 * Outputs sized for the worst case (B*m rows): matching_idxs [K][2] (keypoint index in image 0, in image 1),
 * batch_indexes [K], confidence [K], mlafs0/mlafs1 [K][2][3], keypoints0/1 [K][2]; K is written to count_dev.
 * workspace: og_compact_workspace_bytes. */
size_t og_compact_workspace_bytes(int32_t batch, int32_t m);
int og_compact_matches(const int64_t* matches0, const float* matching_scores0, const float* lafs0, const float* lafs1,
                       int32_t batch, int32_t m, int32_t n, int64_t* matching_idxs, int64_t* batch_indexes,
                       float* confidence, float* mlafs0, float* mlafs1, float* keypoints0, float* keypoints1,
                       int32_t* count_dev, void* workspace_dev, void* stream);

/* ---- the training step's supervision: labels before the matcher, the loss after it (matching_module.py:83-105) ---- */

/* models/gt_matches_generation.py generate_gt_matches with utils/misc.py:21-103: ground-truth labels from keypoints0 [B][m][2],
 * keypoints1 [B][n][2] (pixels, 8-byte aligned) and a known transformation.
 * transform 0 'perspective': H [B][3][3] maps image 0 to image 1 (the reverse direction uses its inverse).
 * transform 1 '3d_reprojection': K0, K1, R [B][3][3], T [B][3]; depth0 / depth1 either per keypoint ([B][m], [B][n]: depth*_h = 0)
 *   or a depth map [B][depth*_h][depth*_w] read at the keypoint truncated to int64 (torch indexing: [-size, 0) wraps around).
 *   A depth of |d| <= 1e-8 (torch.isclose against 0) marks the keypoint invalid.
 * Reprojection ([x, y, 1] through the matrices, divided by w + 1e-8; 3x3 inverses by the adjugate), all-pairs nearest neighbours
 * and labels are computed in fp64 without forming any B x m x n matrix.  gt_matches0 [B][m], gt_matches1 [B][n] (int64):
 *   apply_thresholds = 0 (what the reference produces -- its threshold writes land on copies):
 *     gt0[i] = nn0[i] if nn1[nn0[i]] == i else -1;  -2 where keypoint i has no depth;  image 1 likewise.
 *   apply_thresholds = 1 (the rules of gt_matches_generation.py:63-68, as in-place writes in source order): a mutual pair whose
 *     symmetric distance 0.5 (d0[i] + d1[nn0[i]]) exceeds positive_threshold is -2, exceeds negative_threshold is -1; a
 *     non-mutual keypoint within negative_threshold of its neighbour is -2; no depth -2; a mutual keypoint whose neighbour
 *     has no depth -2.
 * status_dev: one int32 the call zeroes and sets to bit 0 / bit 1 when a depth-map index of image 0 / image 1 is out of range
 *   (the reference raises IndexError; here the depth is not read and counts as missing).  Read it after the stream completes.
 * workspace: og_gt_matches_workspace_bytes, 16-byte aligned.  Returns OG_E_FLAG for an unknown transform. */
size_t og_gt_matches_workspace_bytes(int32_t batch, int32_t m, int32_t n);
int og_gt_matches(int32_t batch, int32_t m, int32_t n, const float* keypoints0, const float* keypoints1, int32_t transform,
                  const float* H, const float* K0, const float* K1, const float* R, const float* T,
                  const float* depth0, int32_t depth0_h, int32_t depth0_w, const float* depth1, int32_t depth1_h, int32_t depth1_w,
                  int32_t apply_thresholds, double positive_threshold, double negative_threshold,
                  int64_t* gt_matches0, int64_t* gt_matches1, int32_t* status_dev, void* workspace_dev, void* stream);

/* utils/losses.py criterion.  scores [B][m+1][n+1] (log-assignment with dustbins), gt_matches0 [B][m], gt_matches1 [B][n] (int64:
 * j >= 0 matched, -1 unmatched, anything else ignored).  losses[0] = the NLL 'loss': per pair the mean of -scores over the
 * matched entries + 0.5 (mean over unmatched0 at the dustbin column + mean over unmatched1 at the dustbin row), an empty set
 * contributing 0, summed over pairs in order and divided by B.  with_margin != 0: losses[1] = 'metric_loss' on the channel-first
 * context_descriptors0 [B][D][m] / 1 [B][D][n] (read in place): dist = 0.5 (1 - a^.b^) on the F.normalize'd columns (exact-fp32
 * MFMA Gram matrix, no B x m x n buffer), triplet terms max(0, d_ap - d_an + margin) against the closest non-positive in the row
 * and in the column of each matched pair, hinge terms max(0, margin - d_an) for the unmatched keypoints of either image, averaged
 * per pair like the NLL; with_margin = 0: losses[1] = 0 and the descriptors are not read (may be NULL).  Both values are
 * bit-identical from run to run.  workspace: og_criterion_workspace_bytes (same with_margin), 16-byte aligned; it carries what
 * og_criterion_backward needs, so keep it until then. */
size_t og_criterion_workspace_bytes(int32_t batch, int32_t m, int32_t n, int32_t with_margin);
int og_criterion_forward(const float* scores, const int64_t* gt_matches0, const int64_t* gt_matches1,
                         const float* context_descriptors0, const float* context_descriptors1,
                         int32_t batch, int32_t m, int32_t n, int32_t D, int32_t with_margin, float margin,
                         float* losses, void* workspace_dev, void* stream);
/* Gradients of grad_losses[0] * loss + grad_losses[1] * metric_loss (grad_losses: device [2], NULL = both 1), with the inputs
 * and the workspace of the forward call.  grad_scores [B][m+1][n+1] (NULL: skipped) is written densely: zero except
 * -w / B at the labelled entries and -0.5 w / B at the dustbin entries (w = 1 / set size).  grad_context_descriptors0/1
 * ([B][D][m], [B][D][n]; both or neither, with_margin only) are written in full; their O(m + n) scattered contributions are
 * float atomics, so they may differ in the last bits from run to run. */
int og_criterion_backward(const int64_t* gt_matches0, const int64_t* gt_matches1,
                          const float* context_descriptors0, const float* context_descriptors1,
                          int32_t batch, int32_t m, int32_t n, int32_t D, int32_t with_margin, float margin,
                          const float* grad_losses, const void* workspace_dev, float* grad_scores,
                          float* grad_context_descriptors0, float* grad_context_descriptors1, void* stream);

/* ABI v12 -- utils/metrics.py, the validation metrics (models/matching_module.py:107-131).  Pairs in the layout SuperGlue.match
 * returns: keypoints0 [B][m][2], keypoints1 [B][n][2] (fp32 pixels, 8-byte aligned), matches0 [B][m] (int64; a keypoint i is
 * matched when i < num_keypoints0[b] and 0 <= matches0[i] < n), num_keypoints0 [B] int32 (NULL: m), K0, K1, R [B][3][3] and
 * T [B][3] (fp32; camera 0 at the identity).  No entry synchronises with the host; each launches a fixed number of kernels.
 *
 * og_epipolar_precision: AccuracyUsingEpipolarDist.  Calibrated points (x - c) / f, E = [T]x R, the squared symmetric epipolar
 *   distance (x1^T E x0)^2 (1 / ((E x0)_0^2 + (E x0)_1^2) + 1 / ((E^T x1)_0^2 + (E^T x1)_1^2)) in fp64; a match is correct when
 *   it is < threshold.  precision = correct / matched, matching_score = correct / num_keypoints0 (both 0 without matches),
 *   num_correct [B].  One kernel. */
int og_epipolar_precision(int32_t batch, int32_t m, int32_t n, const float* keypoints0, const float* keypoints1,
                          const int64_t* matches0, const int32_t* num_keypoints0, const float* K0, const float* K1,
                          const float* R, const float* T, double threshold, float* precision, float* matching_score,
                          int32_t* num_correct, void* stream);
/* og_essential_5pt: the five-point minimal solver (Nister / Stewenius), fp64.  x0, x1 [count][5][2] calibrated correspondences
 *   (x1^T E x0 = 0) -> E [count][10][9] (row-major, unit Frobenius norm; the slots past num_solutions[p] are scratch) and
 *   num_solutions [count] int32 (0..10).  Two kernels; E doubles as their scratch, so no workspace. */
int og_essential_5pt(int32_t count, const double* x0, const double* x1, double* E, int32_t* num_solutions, void* stream);
/* og_relative_pose: CameraPoseAUC's pose.  RANSAC over the five-point solver in calibrated space: `hypotheses` samples of 5
 *   distinct matches drawn by a counter-based hash of (seed, pair_offset + b, hypothesis), every solution scored by the squared
 *   Sampson error <= thr^2, thr = 2 ransac_threshold / mean(K0[0][0] + K1[0][0], K0[1][1] + K1[1][1]) (fp32); the model with
 *   the most inliers wins, the lowest (hypothesis, solution) on ties, so every output is identical from run to run.  Then
 *   kornia's cheirality choice among (R1, t), (R1, -t), (R2, t), (R2, -t) over the inliers, and the error against (R, T):
 *   error [B] = max(rotation error, translation error) in degrees (inf with fewer than 5 matches or no model), R_pred [B][3][3],
 *   t_pred [B][3] (unit; zeros without a model), inliers [B][m] uint8, num_inliers [B] int32.  workspace:
 *   og_relative_pose_workspace_bytes, 16-byte aligned.  10 hypotheses <= 2^30 and batch * hypotheses <= 2^30.  Five kernels. */
size_t og_relative_pose_workspace_bytes(int32_t batch, int32_t m, int32_t hypotheses);
int og_relative_pose(int32_t batch, int32_t m, int32_t n, const float* keypoints0, const float* keypoints1,
                     const int64_t* matches0, const int32_t* num_keypoints0, const float* K0, const float* K1,
                     const float* R, const float* T, float ransac_threshold, int32_t hypotheses, uint64_t seed,
                     int64_t pair_offset, float* error, float* R_pred, float* t_pred, uint8_t* inliers,
                     int32_t* num_inliers, void* workspace_dev, void* stream);

/* Uncalibrated geometric verification (csrc/geometry.hip): what inference.py takes from cv2.findFundamentalMat.  Added to ABI v14
 * without a version bump: three new entries, nothing existing changes.  Pairs in the layout of the metrics above (keypoints in
 * pixels, matches0 with the same validity rule); x1^T F x0 = 0 with x0 from keypoints0.
 *
 * og_fundamental_7pt: the seven-point minimal solver, fp64.  x0, x1 [count][7][2] correspondences with coordinates of order 1 (e.g.
 *   Hartley-normalised) -> F [count][3][9] (row-major, unit Frobenius norm, in ascending order of the cubic's root, the root at infinity
 *   last; the slots past num_solutions[p] are zero) and num_solutions [count] int32 (0..3).  A model is kept when the seven
 *   constraints and det F hold to 1e-9.  One kernel, no workspace.  OG_E_INVALID for count <= 0 or count > 2^30.
 * og_fundamental_matrix: per pair, Hartley normalisation of the valid matches (fp64), `hypotheses` samples of 7 distinct matches drawn
 *   by the counter-based hash of (seed, pair_offset + b, hypothesis) as og_relative_pose draws its 5, every solution scored by the
 *   squared Sampson error in pixels^2 <= threshold^2 (fp32); most inliers win, the lowest (hypothesis, solution) on ties.  Then
 *   `refine` rounds (0: none) of a normalised eight-point least-squares fit to the current inliers with rank 2 enforced, each kept if
 *   it has no fewer inliers, skipped below 8 inliers.  F [B][3][3] fp64 in pixels, unit Frobenius norm, largest entry positive;
 *   inliers [B][m] uint8 at the positions of keypoints0; num_inliers [B]; best_model [B] = hypothesis * 3 + solution of the RANSAC
 *   winner.  With fewer than 7 valid matches or no model: F = 0, no inliers, best_model = -1.  workspace:
 *   og_fundamental_matrix_workspace_bytes, 16-byte aligned.  OG_E_INVALID for hypotheses <= 0, 3 batch hypotheses > 2^30 (the
 *   workspace size is then 0), refine < 0 or a negative threshold.  Four kernels, no host synchronisation, bit-identical from run to run. */
int og_fundamental_7pt(int32_t count, const double* x0, const double* x1, double* F, int32_t* num_solutions, void* stream);
size_t og_fundamental_matrix_workspace_bytes(int32_t batch, int32_t m, int32_t hypotheses);
int og_fundamental_matrix(int32_t batch, int32_t m, int32_t n, const float* keypoints0, const float* keypoints1,
                          const int64_t* matches0, const int32_t* num_keypoints0, float threshold, int32_t hypotheses,
                          int32_t refine, uint64_t seed, int64_t pair_offset, double* F, uint8_t* inliers,
                          int32_t* num_inliers, int32_t* best_model, void* workspace_dev, void* stream);

/* Planar geometric verification and the validation metrics of the homography pre-training stage (csrc/homography.hip): what a user
 * takes from cv2.findHomography, and the perspective counterparts of og_epipolar_precision and og_relative_pose's error.  Added to
 * ABI v14 without a version bump: five new entries, nothing existing changes.  Pairs in the layout of the metrics above; x1 ~ H x0
 * with x0 from keypoints0, H row-major.
 *
 * og_homography_4pt: the four-point minimal solver, fp64.  x0, x1 [count][4][2] correspondences with coordinates of order 1 (e.g.
 *   Hartley-normalised) -> H [count][9] (unit Frobenius norm, largest-magnitude entry positive; zero when num_solutions[p] is 0) and
 *   num_solutions [count] int32 (0 or 1).  A model is kept when each of the four point triples has a signed area above 1e-9 in both
 *   images with the same sign in both (cv2's orientation test, which removes collinear triples too), all nine entries are finite and
 *   the eight DLT constraints hold to 1e-9.  One kernel, no workspace.  OG_E_INVALID for count <= 0 or count > 2^30.
 * og_homography: per pair, Hartley normalisation of the valid matches (fp64, as og_fundamental_matrix), `hypotheses` samples of 4
 *   distinct matches drawn by the counter-based hash of (seed, pair_offset + b, hypothesis), every model scored by the squared forward
 *   transfer error |proj(H, x0) - x1|^2 in pixels^2 <= threshold^2 (fp32; a non-finite error is an outlier); most inliers win, the
 *   lowest hypothesis on ties.  Then `refine` rounds (0: none) of a normalised DLT least-squares fit to the current inliers, each kept
 *   if it is finite and has no fewer inliers, skipped below 5 inliers.  H [B][3][3] fp64 in pixels, unit Frobenius norm, largest
 *   entry positive; inliers [B][m] uint8 at the positions of keypoints0; num_inliers [B]; best_model [B] = hypothesis of the RANSAC
 *   winner.  With fewer than 4 valid matches or no model: H = 0, no inliers, best_model = -1.  workspace:
 *   og_homography_workspace_bytes, 16-byte aligned (OG_E_ALIGN).  OG_E_INVALID for hypotheses <= 0, batch hypotheses > 2^30 (the
 *   workspace size is then 0), refine < 0 or a negative or NaN threshold.  Four kernels, no host synchronisation, bit-identical from
 *   run to run.
 * og_homography_precision: H_true [B][3][3] fp32.  For every valid match |proj(H_true, keypoints0[i]) - keypoints1[matches0[i]]| in
 *   fp64; a match is correct when it is < threshold (pixels).  precision = correct / matched, matching_score = correct /
 *   num_keypoints0 (both 0 without matches), num_correct [B].  One kernel.
 * og_homography_corner_error: error [B] fp32 = the mean distance in pixels between the four corners (0, 0), (0, height - 1),
 *   (width - 1, 0), (width - 1, height - 1) mapped by H_est [B][3][3] fp64 and by H_true [B][3][3] fp32, in fp64; +inf for an
 *   all-zero estimate or a non-finite projection.  One kernel.  OG_E_INVALID for width or height <= 0. */
int og_homography_4pt(int32_t count, const double* x0, const double* x1, double* H, int32_t* num_solutions, void* stream);
size_t og_homography_workspace_bytes(int32_t batch, int32_t m, int32_t hypotheses);
int og_homography(int32_t batch, int32_t m, int32_t n, const float* keypoints0, const float* keypoints1, const int64_t* matches0,
                  const int32_t* num_keypoints0, float threshold, int32_t hypotheses, int32_t refine, uint64_t seed,
                  int64_t pair_offset, double* H, uint8_t* inliers, int32_t* num_inliers, int32_t* best_model, void* workspace_dev,
                  void* stream);
int og_homography_precision(int32_t batch, int32_t m, int32_t n, const float* keypoints0, const float* keypoints1,
                            const int64_t* matches0, const int32_t* num_keypoints0, const float* H_true, float threshold,
                            float* precision, float* matching_score, int32_t* num_correct, void* stream);
int og_homography_corner_error(int32_t batch, const double* H_est, const float* H_true, int32_t width, int32_t height, float* error,
                               void* stream);

/* Sigma-consensus scoring (MAGSAC++, what cv2.USAC_MAGSAC scores with) for the two estimators above (the _sc entries in csrc/geometry.hip
 * and csrc/homography.hip, og_sigma_consensus_eval in csrc/sigma_consensus.hip).  Added to ABI v14 without a version bump: three new entries, nothing existing
 * changes.  Constants as OpenCV's: 4 degrees of freedom, a = 1.5, k = 3.64, sigma_max = threshold / k, u_max = k^2 / 2.  With e a
 * match's squared residual (pixels^2: Sampson for F, forward transfer for H), t = e / threshold^2 and u = t u_max,
 *   w(t) = (G(a, u) - G(a, u_max)) / (G(a) - G(a, u_max)),   q(t) = 1 - (g(a + 1, u) + u (G(a, u) - G(a, u_max))) / g(a + 1, u_max)
 * (G / g the upper / lower incomplete gamma function) for t <= 1, both 0 otherwise; a match with `e <= threshold^2` false (NaN and
 * infinity included) contributes nothing, and threshold = 0 takes t = 0 for e = 0.  `threshold` is here an upper bound on the
 * noise, not a decision boundary: below about twice the noise the weights are too tight.
 *
 * og_fundamental_matrix_sc / og_homography_sc: og_fundamental_matrix / og_homography with a model scored by
 *   Q = sum over its valid matches of rint(65536 q(t)) (an integer: the winner does not depend on the order of summation); the largest
 *   Q wins, the lowest model on ties.  The refits are the same least-squares fits over the matches with e <= threshold^2, each
 *   match's rows weighted by w(t) under the current model; a refit is kept if it is finite and its Q is no smaller, and a round is
 *   skipped below 8 (F) / 5 (H) such matches.  inliers, num_inliers: e <= threshold^2 under the final model, as in the plain entries;
 *   quality [B] fp32 = Q / 65536 of the final model, the soft inlier count, 0 without a model.  Same workspace
 *   (og_fundamental_matrix_workspace_bytes / og_homography_workspace_bytes), same draws, same refusals, and OG_E_SHAPE for m > 32768
 *   (Q + 1 must fit 32 bits).  Four kernels, no host synchronisation, bit-identical from run to run.
 * og_sigma_consensus_eval: t [count] fp32 -> q [count] uint32 = rint(65536 q(t)) within one unit, non-increasing in t, and w [count]
 *   fp32 within 1.5e-6; (0, 0) for t outside [0, 1] and for NaN, (65536, 1) at t = 0.  The device function the kernels above score
 *   with.  One kernel.  OG_E_INVALID for count <= 0 or count > 2^30. */
int og_fundamental_matrix_sc(int32_t batch, int32_t m, int32_t n, const float* keypoints0, const float* keypoints1,
                             const int64_t* matches0, const int32_t* num_keypoints0, float threshold, int32_t hypotheses,
                             int32_t refine, uint64_t seed, int64_t pair_offset, double* F, uint8_t* inliers,
                             int32_t* num_inliers, int32_t* best_model, float* quality, void* workspace_dev, void* stream);
int og_homography_sc(int32_t batch, int32_t m, int32_t n, const float* keypoints0, const float* keypoints1, const int64_t* matches0,
                     const int32_t* num_keypoints0, float threshold, int32_t hypotheses, int32_t refine, uint64_t seed,
                     int64_t pair_offset, double* H, uint8_t* inliers, int32_t* num_inliers, int32_t* best_model, float* quality,
                     void* workspace_dev, void* stream);
int og_sigma_consensus_eval(int32_t count, const float* t, uint32_t* q, float* w, void* stream);

/* ABI v13 -- the SuperPoint detector / descriptor (models/features/superpoint/model.py, SuperPointNet / SuperPointNetBn), inference
 * only (eval-mode BatchNorm, folded at pack time).  descriptor_dim 256.  Image [B][H][W] fp32, H, W >= 8, B * H * W <= 2^26;
 * Hc = H / 8, Wc = W / 8 (floor, as the three 2x2 max-pools), the heatmap is [B][8 Hc][8 Wc].
 *
 * og_superpoint_pack (host): params = 24 host pointers, weight [out][in][3][3 or 1] and bias of conv1a, conv1b, conv2a, conv2b,
 *   conv3a, conv3b, conv4a, conv4b, convPa, convPb, convDa, convDb; with batch_norm != 0 followed by 48 more, weight / bias /
 *   running_mean / running_var of bn1a, bn1b, ..., bn4b, bnPa, bnPb, bnDa, bnDb (BatchNorm eps bn_eps).  Writes
 *   og_superpoint_packed_bytes bytes; OG_E_RANGE if a folded weight is not finite.
 * og_superpoint_dense: image -> heatmap [B][8 Hc][8 Wc] (softmax over 65, dustbin dropped, depth-to-space) and coarse descriptors
 *   [B][Hc][Wc][256] (NHWC, divided by their L2 norm).  Workspace og_superpoint_workspace_bytes, 16-byte aligned; shared with
 *   og_superpoint_detect (the two run one after the other on the stream).
 * og_superpoint_detect: heatmap [B][Hh][Wh] -> NMS (kornia nms2d: replicate padding, strictly greater than the other k*k-1),
 *   > threshold and != 0, remove_borders, top_k_keypoints(max_kpts, -1 = all) and min_stack.  nms_kernel odd, 3..17.
 *   counts[b] = candidates of image b, counts[B + b] = keypoints kept (equal for every b).  sel_idx / sel_score [B][sel_ld]
 *   (sel_ld >= og_superpoint_capacity) receive raster index y * Wh + x and score of each kept keypoint: in raster order when
 *   neither top-k nor min_stack cut (every image keeps the same count, uncut), otherwise by descending score, equal scores
 *   in raster order.
 * og_superpoint_describe: n = counts[B] keypoints per image -> lafs [B][n][2][3] (identity, (x, y)), scores [B][n], descriptors
 *   [B][n][256] (sample_desc_from_points: bilinear, align_corners=False, zero padding, then F.normalize). */
size_t og_superpoint_packed_bytes(int32_t descriptor_dim);
int og_superpoint_pack(int32_t descriptor_dim, int32_t batch_norm, float bn_eps, const float* const* params, void* packed_host);
int og_superpoint_capacity(int32_t H, int32_t W, int32_t max_kpts);
size_t og_superpoint_workspace_bytes(int32_t batch, int32_t H, int32_t W, int32_t nms_kernel, int32_t max_kpts);
int og_superpoint_dense(int32_t batch, int32_t H, int32_t W, const float* image, const void* packed_dev, float* heatmap,
                        float* coarse_desc, void* workspace_dev, void* stream);
int og_superpoint_detect(int32_t batch, int32_t Hh, int32_t Wh, int32_t nms_kernel, int32_t border, float threshold, int32_t max_kpts,
                         const float* heatmap, int32_t* counts, int32_t* sel_idx, float* sel_score, int64_t sel_ld,
                         void* workspace_dev, void* stream);
int og_superpoint_describe(int32_t batch, int32_t Hc, int32_t Wc, int32_t n, const int32_t* sel_idx, const float* sel_score,
                           int64_t sel_ld, const float* coarse_desc, float* lafs, float* scores, float* descriptors, void* stream);

/* Fine-tuning SuperPointNet (no BatchNorm, descriptor_dim 256): the training forward and the backward of the extractor
 * (csrc/superpoint_train.hip; models/matching_module.py `finetune: True`).  Exact fp32, no atomics: gradients are bit-identical from
 * run to run.  Additive to ABI v14.
 *
 * og_superpoint_train_forward: og_superpoint_dense (same packed blob, same heatmap and coarse descriptors bit for bit) that keeps
 *   the post-ReLU output of every 3x3 layer in `saved` (og_superpoint_train_saved_bytes, 16-byte aligned).  `saved` begins with the
 *   hidden map of the two heads, [B Hc Wc][512] (convPa | convDa after ReLU).
 * og_superpoint_train_pack (host): params as og_superpoint_pack (24 pointers) -> the data-gradient blob,
 *   og_superpoint_train_packed_bytes bytes: for layer j = conv1b, 2a, 2b, 3a, 3b, 4a, 4b, heads (convPa | convDa as one layer of 512
 *   output channels) in this order a block of Cout * 9 * Cin floats, the weights transposed and the taps flipped in the fragment-major
 *   layout of the forward blob: [ci / 32][step][lane][4], step = ((co / 32) * 9 + tap') * 4 + kk, lane l element e holding
 *   W[co = 32 (co / 32) + 8 kk + 4 (l >> 5) + e][ci = 32 (ci / 32) + (l & 31)][tap = 8 - tap'].
 * og_superpoint_train_backward: g_hidden [B Hc Wc][512] = the gradient of the heads' hidden map BEFORE its ReLU ->  `grads`, flat:
 *   conv1a weight [64][9], bias [64], then per layer j weight [Cout][Cin][9] (torch's order) and bias [Cout]; heads rows 0..255 are
 *   convPa, 256..511 convDa.  first_layer: 0 = conv1a, 1 + j = layer j; layers below it are neither computed nor written.
 *   layer_grads (debug, may be NULL): receives, for every layer j visited, the gradient of its pre-activation output at the layer's
 *   own resolution as the kernels form it (pool routing applied), [B][h_j][w_j][Cout_j] one after the other for j = 0..7.
 *   Workspace og_superpoint_train_workspace_bytes(batch, H, W, n), 16-byte aligned, shared with og_superpoint_describe_backward.
 * og_superpoint_describe_backward: d_descriptors [B][n][256] -> d_coarse [B][Hc][Wc][256], the gradient of the coarse (normalised)
 *   descriptors through F.normalize and the bilinear sampling; each cell gathers from the keypoints that touch it, in keypoint order.
 *   n >= 1. */
size_t og_superpoint_train_packed_bytes(int32_t descriptor_dim);
int og_superpoint_train_pack(int32_t descriptor_dim, const float* const* params, void* packed_host);
size_t og_superpoint_train_saved_bytes(int32_t batch, int32_t H, int32_t W);
size_t og_superpoint_train_workspace_bytes(int32_t batch, int32_t H, int32_t W, int32_t n);
int og_superpoint_train_forward(int32_t batch, int32_t H, int32_t W, const float* image, const void* packed_dev, void* saved_dev,
                                float* heatmap, float* coarse_desc, void* stream);
int og_superpoint_train_backward(int32_t batch, int32_t H, int32_t W, const float* image, const void* packed_grad_dev,
                                 const void* saved_dev, const float* g_hidden, int32_t first_layer, float* grads, float* layer_grads,
                                 void* workspace_dev, void* stream);
int og_superpoint_describe_backward(int32_t batch, int32_t Hc, int32_t Wc, int32_t n, const int32_t* sel_idx, int64_t sel_ld,
                                    const float* coarse_desc, const float* d_descriptors, float* d_coarse, void* workspace_dev,
                                    void* stream);

/* Fine-tuning SuperPointNetBn: train-mode BatchNorm2d behind every convolution (csrc/superpoint_bn_train.hip; reference
 * models/features/superpoint/model.py:180-199 with the modules in train()).  Exact fp32, no atomics, every sum in a fixed order.
 * Additive to ABI v14.  B * (H / 8) * (W / 8) >= 2: one value per channel has no batch variance (the byte queries return 0).
 *
 * og_superpoint_bn_train_forward: packed_dev = the blob of og_superpoint_pack(..., batch_norm = 0, ...): the RAW weights.  bn (host
 *   array of 40 device pointers): weight, bias, running_mean, running_var of bn1a, bn1b, bn2a, ..., bn4b, bnPa, bnDa in this order;
 *   eps, momentum (host, 10 floats): per module.  Every layer's batch statistics are taken over the B h w pixels it convolves at, the
 *   running buffers are updated in place (running_var with the unbiased variance), like torch.  `saved`
 *   (og_superpoint_bn_train_saved_bytes, 16-byte aligned) begins with the hidden map of the two heads, [B Hc Wc][512]:
 *   relu(bnPa(convPa)) | relu(bnDa(convDa)).  convPb / bnPb / convDb / bnDb are the caller's (og_gemm_nt, og_batchnorm_train_*), then:
 * og_superpoint_bn_cell_tail: logits [B Hc Wc][ld_logits] (65 used, after bnPb) -> softmax, dustbin dropped, depth-to-space ->
 *   heatmap [B][Hc*8][Wc*8]; desc_raw [B Hc Wc][256] (after bnDb) -> coarse_desc, unit L2 norm per cell.
 * og_superpoint_bn_train_backward: g_hidden = the gradient of the hidden map AFTER its ReLU (the mask is applied here, from the saved
 *   raw output).  packed_grad_dev, first_layer, grads and workspace alignment as og_superpoint_train_backward; the bias slots of `grads`
 *   are not written (the mean subtraction removes the convolution biases: their gradient is zero).  bn_grads [2][1280]: d weight then
 *   d bias of the BatchNorm layers, channels in the order bn1a (64), bn1b, bn2a, bn2b (64 each), bn3a, bn3b, bn4a, bn4b (128 each),
 *   bnPa | bnDa (512); written for every layer visited (layer j's BatchNorm with layer j; bn1a when first_layer == 0).
 *   layer_grads (debug, may be NULL): dz = the gradient of the raw convolution output, dense, [B][H][W][64] of conv1a first and then
 *   [B][h_j][w_j][Cout_j] for j = 0..7.  One workspace (og_superpoint_bn_train_workspace_bytes, 16-byte aligned) serves both calls. */
size_t og_superpoint_bn_train_saved_bytes(int32_t batch, int32_t H, int32_t W);
size_t og_superpoint_bn_train_workspace_bytes(int32_t batch, int32_t H, int32_t W);
int og_superpoint_bn_train_forward(int32_t batch, int32_t H, int32_t W, const float* image, const void* packed_dev, float* const* bn,
                                   const float* eps, const float* momentum, void* saved_dev, void* workspace_dev, void* stream);
int og_superpoint_bn_cell_tail(int32_t batch, int32_t Hc, int32_t Wc, const float* logits, int64_t ld_logits, const float* desc_raw,
                               float* heatmap, float* coarse_desc, void* stream);
int og_superpoint_bn_train_backward(int32_t batch, int32_t H, int32_t W, const float* image, const void* packed_grad_dev,
                                    const void* saved_dev, const float* g_hidden, int32_t first_layer, float* grads, float* bn_grads,
                                    float* layer_grads, void* workspace_dev, void* stream);

/* ABI v14 -- the reference's optimizer step: torch.optim.Adam + StepLR(step_size=1) stepped every iteration (models/matching_module.py:133-147)
 * behind torch.nn.utils.clip_grad_norm_ (train.py:73 gradient_clip_val), fused into three launches whatever the number of parameters
 * (csrc/optimizer.hip).  The caller owns three flat fp32 device buffers grad / exp_avg / exp_avg_sq of layout.total floats in which
 * parameter i has the segment [offsets[i], offsets[i] + numel[i]); every offset is a multiple of 4, the padding between segments is zero and is
 * never written.  The parameters themselves stay where they are (16-byte aligned device pointers).
 *
 * og_adam_layout (host arithmetic only): from the numel list, offsets [count] (may be NULL), the chunk map (may be NULL: sizes only;
 *   else 2 * num_chunks int32, {parameter index, chunk index within the parameter} per update workgroup -- parameter i is cut into
 *   ceil(numel[i] / OG_ADAM_CHUNK) chunks of OG_ADAM_CHUNK floats) and the sizes.  OG_E_INVALID for an empty list or a numel <= 0.
 * og_adam_step: one step.  params: HOST array of the count parameter pointers (checked: NULL -> OG_E_INVALID, not 16-byte aligned ->
 *   OG_E_ALIGN); table_dev: the same on the DEVICE, count rows of three 8-byte words {pointer, offset, numel} (layout.table_bytes);
 *   chunk_map_dev: the chunk map on the device; workspace_dev: layout.workspace_bytes bytes, 8-byte aligned, whose first OG_ADAM_SCALARS
 *   doubles are the scalars block below -- zero it once, it carries the step count from call to call (set OG_ADAM_STEP to resume).
 *     clip != 0: adam_gradnorm_kernel (fp32 squares of the flat gradient summed in fp64, one partial per OG_ADAM_NORM_CHUNK floats, no
 *       atomics), then adam_prepare_kernel: total_norm = sqrt(sum of the partials in a fixed order), clip_coef = min(1, max_norm /
 *       (total_norm + 1e-6)).  clip == 0: no norm launch, total_norm = NaN, clip_coef = 1.
 *     step += 1; lr_t = lr gamma^(step-1); step_size = lr_t / (1 - beta1^step); all scalar arithmetic in fp64.
 *     adam_update_kernel, per element in fp32, every operation rounded on its own as torch's kernels round it:
 *       g = clip_coef g; m = m + (1-beta1)(g - m); v = beta2 v + (1-beta2) g g; p = p - step_size m / (sqrt(v) / sqrt(1-beta2^step) + eps);
 *       p, m, v are stored and g = 0 is written: the next backward accumulates into zeros.
 *   Every parameter takes part in every step (a zero gradient is a gradient).  No host synchronisation, no copy, no atomics: results are
 *   bit-identical from run to run. */
#define OG_ADAM_CHUNK         4096
#define OG_ADAM_NORM_CHUNK    8192
#define OG_ADAM_SCALARS       8      /* doubles at the head of the workspace: */
#define OG_ADAM_TOTAL_NORM    0      /*   gradient norm before clipping (NaN when clip == 0)   */
#define OG_ADAM_CLIP_COEF     1
#define OG_ADAM_STEP          2      /*   steps taken so far                                   */
#define OG_ADAM_LR            3      /*   lr_t of the last step                                */
#define OG_ADAM_STEP_SIZE     4
#define OG_ADAM_INV_SQRT_BC2  5
typedef struct og_adam_layout_t {
    int64_t total;            /* floats of each flat buffer (multiple of 4)                    */
    int64_t table_bytes;      /* device table: count rows of 24 bytes                          */
    int64_t workspace_bytes;  /* scalars block + norm partials                                 */
    int32_t num_chunks;       /* update workgroups = rows of the chunk map                     */
    int32_t num_partials;     /* norm workgroups                                               */
    int32_t chunk;            /* OG_ADAM_CHUNK                                                 */
    int32_t reserved;
} og_adam_layout_t;
int og_adam_layout(int32_t count, const int64_t* numel, int64_t* offsets, int32_t* chunk_map, og_adam_layout_t* layout);
int og_adam_step(int32_t count, const void* const* params, const void* table_dev, const int32_t* chunk_map_dev, int32_t num_chunks,
                 int64_t total, float* grad, float* exp_avg, float* exp_avg_sq, double* workspace_dev, double lr, double gamma,
                 double beta1, double beta2, double eps, int32_t clip, double max_norm, void* stream);

/* ABI v14, additive -- the SIFT keypoint extractor (csrc/sift.hip): DoG detector and SIFT / RootSIFT descriptor, a drop-in for the
 * reference's OPENCV_SIFT features (models/features/opencv/): Lowe 2004 with OpenCV's constants (3 layers per octave, sigma 1.6, first
 * octave -1, assumed input blur 0.5), the contrast and edge tests off as the reference sets them, then the reference's own radius NMS,
 * top-k, LAFs and descriptor normalisation (base.py).  Not bit-identical to cv2.SIFT_create; tests/sift_ref.py is the specification.
 * Limits: 8 <= H, W <= 8192 and B * H * W <= 2^22; anything else (a null pointer included) returns OG_E_INVALID, og_sift_workspace_bytes 0.
 *
 * Geometry (og_sift_geometry, host arithmetic): out[0] = octaves built, out[1] = cap, the keypoint capacity per image (max(1024,
 *   H W / 2)), out[2] = cap2 = cap + cap / 4, the capacity after one keypoint per orientation; out[3 + 2 o], out[4 + 2 o] = h, w of
 *   octave o (2H x 2W, halved with floor; octaves with a side below 11 are not built); 35 ints.  Per image, gauss is
 *   [octave][6][h][w] and dog [octave][5][h][w], octaves packed one after the other.  The select stage holds 32 cap2 neighbour entries.
 * counts, int32 [4 B + 1], is filled along the way: [b] keypoints detected, [B + b] oriented keypoints, [2 B + b] kept after NMS and
 *   top-k, [3 B + b] neighbour-list entries, [4 B] = min_b counts[2 B + b], the rows every image puts out (min_stack).  A count above
 *   its capacity means the buffers were too small for this image: the stages stay in bounds and process the first cap / cap2, the
 *   caller must treat it as an error (openglue_amd/sift.py raises).
 * All stages of one call share one workspace (og_sift_workspace_bytes, 16-byte aligned) and run in order on one stream.
 *
 * og_sift_pyramid: image [B][H][W] in [0, 1] -> u = clamp(trunc(255.f x), 0, 255), bilinear 2x (pixel-centre aligned), blur
 *   sqrt(1.6^2 - 1), then per octave 6 incrementally blurred images (radius (round(8 s + 1) | 1) / 2, fp64-normalised fp32 taps,
 *   reflect-101, rows then columns, fp32) and their 5 differences; the next octave starts from every second pixel of image 3.
 * og_sift_detect: extrema of DoG layers 1..3 inside a 5-pixel border (> 0 and >= all 26 neighbours, or < 0 and <= all), refined in
 *   fp64 by up to 5 Newton steps.  det_i [B][cap][4] = octave, layer, row, column of the converged sample; det_f [B][cap][4] (double) =
 *   x, y in input pixels ((c + x_c) 2^(o-1) - 0.25), size = 2 * 1.6 * 2^((l + x_l) / 3) * 2^(o-1), response |D + grad . x / 2| / 255.
 *   Order: octave, layer, row, column of the extremum each started from.
 * og_sift_orient: 36-bin gradient histogram (radius round(4.5 s), weight std 1.5 s, [1 4 6 4 1] / 16 smoothing), one keypoint per
 *   local peak >= 0.8 max by descending height, parabolic interpolation; upright != 0: angle 0.  ori_i [B][cap2][6] = octave, layer,
 *   row, column, orientation rank, source keypoint; ori_f [B][cap2][5] (float) = x, y, size, angle in degrees [0, 360), response.
 * og_sift_describe: desc [B][cap2][128], [row bin][column bin][orientation bin]: bin width 3 s, Gaussian window of 2 bins, trilinear;
 *   L2-normalise, clip 0.2, renormalise, quantize != 0: min(255, round(512 v)); then rootsift > 0: L1-normalise and square root,
 *   0: L2-normalise, < 0: left as it is (the bytes).  An all-zero descriptor stays zero.
 * og_sift_select: greedy radius NMS in descending response (radius nms_diameter / 2, distance <= radius; <= 0: none), then the
 *   max_kpts strongest (<= 0: all).  sel [B][cap2] = indices into ori_* in output order: descending response, equal ones by (octave,
 *   layer, row, column, orientation rank), then index.  Equal to the sequential greedy pass.
 * og_sift_gather: n = counts[4 B] -> lafs [B][n][2][3] (scale 6 size, angle deg2rad(-angle)), scores [B][n], descriptors [B][n][128]. */
int og_sift_geometry(int32_t H, int32_t W, int32_t* out);
size_t og_sift_workspace_bytes(int32_t batch, int32_t H, int32_t W);
int og_sift_pyramid(int32_t batch, int32_t H, int32_t W, const float* image, float* gauss, float* dog, void* workspace_dev, void* stream);
int og_sift_detect(int32_t batch, int32_t H, int32_t W, const float* dog, int32_t* det_i, double* det_f, int32_t* counts,
                   void* workspace_dev, void* stream);
int og_sift_orient(int32_t batch, int32_t H, int32_t W, int32_t upright, const float* gauss, const int32_t* det_i, const double* det_f,
                   int32_t* counts, int32_t* ori_i, float* ori_f, void* workspace_dev, void* stream);
int og_sift_describe(int32_t batch, int32_t H, int32_t W, int32_t quantize, int32_t rootsift, const float* gauss, const int32_t* ori_i,
                     const float* ori_f, const int32_t* counts, float* desc, void* stream);
int og_sift_select(int32_t batch, int32_t H, int32_t W, float nms_diameter, int32_t max_kpts, const int32_t* ori_i, const float* ori_f,
                   int32_t* counts, int32_t* sel, void* workspace_dev, void* stream);
int og_sift_gather(int32_t batch, int32_t H, int32_t W, int32_t n, const int32_t* sel, const float* ori_f, const float* desc,
                   float* lafs, float* scores, float* descriptors, void* stream);

/* ABI v14, additive -- the patch networks behind the DoG detector (csrc/patchnet.hip): the reference's OPENCVDoGAffNetHardNet
 * (models/features/opencv/dog_affnet_harnet.py) after its detector: lafs = orinet(affnet(lafs, image), image), 32 x 32 patches from an
 * image pyramid, HardNet descriptors.  A kornia 0.6-era reading, pinned by tests/patchnet_ref.py; exact fp32, deterministic.
 * kind: 0 HardNet (1-32-32-64-64-128-128, 128 outputs), 1 AffNet (1-16-16-32-32-64-64, 3 outputs), 2 OriNet (as AffNet, 2 outputs).
 * Limits: 1 <= H, W <= 8192 and B * H * W <= 2^22, n <= 2^24; anything else (a null pointer included) returns OG_E_INVALID.
 *
 * og_patch_geometry (host): out[0] = pyramid levels (built while min(h, w) >= 32, at most 12), out[1] = floats per image, out[2 + 2 l],
 *   out[3 + 2 l] = h, w of level l (halved with floor); 26 ints.  The pyramid buffer is [level][B][h][w], levels one after the other.
 * og_patch_workspace_bytes: one scratch for og_patch_pyramid on [batch][H][W] and og_patchnet_forward on n patches (either part may
 *   be all zeros); 16-byte aligned.  0: unsupported.
 * og_patch_pyramid: level l + 1 = level l blurred with [1 4 6 4 1] x [1 4 6 4 1] / 256 (reflect border, no edge repeat), resized
 *   bilinearly (align_corners false) to half size.
 * og_patch_extract: lafs [B][n][2][3] -> patches [B n][32][32].  Level max(0, floor(log2(2 scale / 32))), scale = sqrt |det A|; a level
 *   that was not built gives a zero patch; bilinear, border clamp.  upright != 0: A is replaced by scale * I.  normalize != 0:
 *   (x - mean) / (std + 1e-6) per patch, unbiased std.
 * og_patchnet_pack (host): params = host pointers: weight, BatchNorm running_mean, running_var of features.0 / 3 / 6 / 9 / 12 / 15 (18),
 *   features.19.weight, then HardNet: features.20 running_mean, running_var; AffNet / OriNet: features.19.bias.  BatchNorm (affine
 *   false) is folded into its convolution.  OG_E_RANGE if a folded weight is not finite.
 * og_patchnet_forward: patches [n][32][32] (normalize != 0: raw patches, normalised here).  HardNet: out [n][128], L2-normalised.
 *   AffNet: out [n][3] (tanh outputs, may be null) and lafs [n][2][3] updated in place (may be null): A = scale(A) A' rot(ori(A)),
 *   A' = [[1 + x0, 0], [x1, 1 + x2]] / sqrt(det).  OriNet: out [n][2], lafs: A = A rot(atan2(y0 + 1e-8, y1 + 1e-8)).
 *   rot(t) = [[cos t, sin t], [-sin t, cos t]]. */
int og_patch_geometry(int32_t H, int32_t W, int32_t* out);
size_t og_patch_workspace_bytes(int32_t batch, int32_t H, int32_t W, int32_t n);
int og_patch_pyramid(int32_t batch, int32_t H, int32_t W, const float* image, float* pyramid, void* workspace_dev, void* stream);
int og_patch_extract(int32_t batch, int32_t H, int32_t W, int32_t n, const float* pyramid, const float* lafs, int32_t upright,
                     int32_t normalize, float* patches, void* stream);
size_t og_patchnet_packed_bytes(int32_t kind);
int og_patchnet_pack(int32_t kind, float bn_eps, const float* const* params, void* packed_host);
int og_patchnet_forward(int32_t kind, int32_t n, const float* patches, int32_t normalize, const void* packed_dev, float* out,
                        float* lafs, void* workspace_dev, void* stream);

/* ABI v14, additive -- homography training pairs (csrc/pairs.hip): the arithmetic of the reference's self-supervised data items,
 * OxfordParis1MDataset.__getitem__ (data/oxford_paris_dataset.py:27-66) and MegaDepthWarpingDataset.__getitem__
 * (data/megadepth_dataset.py:33-52): cv2.getPerspectiveTransform, cv2.warpPerspective (bilinear, constant border 0), crop, grey, / 255.
 * Device pointers only, no host synchronisation, no allocation; every result is bit-identical from run to run and independent of the
 * batch it is computed in.  tests/pairs_ref.py is the specification.  Limits: 1 <= batch <= 65535, 1 <= H, W <= 32768, C in {1, 3};
 * anything else returns OG_E_SHAPE, a null pointer OG_E_INVALID, a matrix pointer that is not 8-byte aligned OG_E_ALIGN.
 *
 * og_perspective_transform: src, dst [batch][4][2] float -> M [batch][3][3] double with M (x, y, 1) ~ (u, v, 1) for the four pairs.
 *   Point i gives row i = [x y 1 0 0 0 -xu -yu | u] and row i + 4 = [0 0 0 x y 1 -xv -yv | v]; the 8 x 8 system is solved in fp64 by
 *   Gaussian elimination with partial pivoting (first largest |entry| of the column) and back substitution, M[2][2] = 1.  A pivot that
 *   is not above 1e-12 times the largest |coefficient| of the system (zero at the level of rounding), or a non-finite result: M = 0.
 * og_warp_perspective_u8: src [batch][H][W][C] bytes, M [batch][3][3] double (source -> destination, as cv2.warpPerspective without
 *   WARP_INVERSE_MAP) -> dst [batch][h][w][C]: the window with origin (x0, y0) and size w x h of the H x W destination frame
 *   (0 <= x0, x0 + w <= W, 0 <= y0, y0 + h <= H, else OG_E_SHAPE).  Per image Mi = adj(M) * (1 / det M) in fp64 (Mi = 0 when det = 0);
 *   per destination pixel (x, y), every fp64 operation rounded on its own:
 *     Wd = (Mi20 x + Mi21 y) + Mi22;  s = Wd != 0 ? 32 / Wd : 0;  fX = ((Mi00 x + Mi01 y) + Mi02) s, fY likewise;
 *     fX > INT_MAX -> INT_MAX, not (fX >= INT_MIN) -> INT_MIN;  X = rint(fX) (half to even), Y likewise;
 *     sx = X >> 5, fx = X & 31, sy = Y >> 5, fy = Y & 31; taps (sy, sx), (sy, sx + 1), (sy + 1, sx), (sy + 1, sx + 1), 0 outside the
 *     source, integer weights 32 (32 - fx)(32 - fy), 32 fx (32 - fy), 32 (32 - fx) fy, 32 fx fy (sum 32768);
 *     out = (sum w v + 16384) >> 15 per channel.
 * og_homography_pairs: frames [batch][H][W][C] bytes, warp_offset [batch][4][2] float -> image0, image1 [batch][1][h][w] float with
 *   h = H - 2 offset, w = W - 2 offset (offset >= 0, 2 offset < min(H, W)), H_true [batch][3][3] float.  With the corners c =
 *   (o, o), (o, H-o-1), (W-o-1, o), (W-o-1, H-o-1): H_warp = transform(c + warp_offset -> c) stays in fp64 in workspace_dev (9 batch
 *   doubles, 8-byte aligned) and drives the warp; H_true = transform(c - o + warp_offset -> c - o) rounded to float.  One launch solves
 *   both systems of every pair, one launch writes both views: image0 = grey(frame window) / 255.f, image1 = grey(warp window) / 255.f,
 *   grey(R, G, B) = (9798 R + 19235 G + 3735 B + 16384) >> 15 on the bytes after the warp (C = 1: the byte itself).
 *   warp_offset == NULL: workspace_dev already holds the batch warp matrices, nothing is solved and H_true is not written (may be NULL). */
int og_perspective_transform(int32_t batch, const float* src, const float* dst, double* M, void* stream);
int og_warp_perspective_u8(int32_t batch, int32_t H, int32_t W, int32_t C, const uint8_t* src, const double* M, int32_t x0, int32_t y0,
                           int32_t w, int32_t h, uint8_t* dst, void* stream);
int og_homography_pairs(int32_t batch, int32_t H, int32_t W, int32_t C, const uint8_t* frames, int32_t offset, const float* warp_offset,
                        float* image0, float* image1, float* H_true, void* workspace_dev, void* stream);

/* ABI v14, additive -- MegaDepth training pairs (csrc/megadepth.hip): the arithmetic of the reference's main-stage data items,
 * MegaDepthPairsDataset.__getitem__ (data/megadepth_dataset.py:119-192), MegaDepthPairsDatasetFeatures.__getitem__ (:203-282) and the collate
 * stack_keypoints_batch (data/megadepth_datamodule.py:105-166): grey, cv2.resize of the image and of its depth map, crop, K; for cached
 * features the crop mask, the selection of num_keypoints keypoints and one depth value per keypoint.  Device pointers only (the tables also
 * in a host copy, which is what gets validated), no host synchronisation, no allocation; every result is bit-identical from run to run and
 * independent of the batch it is computed in.  tests/megadepth_ref.py is the specification.  Limits: every image side and resized side in
 * [1, 32768], at most 65535 images per call, C in {1, 3}; anything else returns OG_E_SHAPE, a null pointer OG_E_INVALID, an unknown
 * interpolation OG_E_FLAG, a float output that is not 16-byte aligned (or a float input not 4-byte aligned) OG_E_ALIGN -- all before
 * anything is launched.
 *
 * The resize of an axis from src to dst: scale = 1.0 / ((double)dst / src); destination index d has f = (float)((d + 0.5) scale - 0.5),
 * s = floor(f), f -= s; s < 0 -> s = 0, f = 0; s >= src - 1 -> s = src - 1, f = 0; taps s and min(s + 1, src - 1).
 * og_resize_linear_u8: src [batch][H][W][C] bytes -> dst [batch][h][w][C], the window with origin (x0, y0) and size w x h of the images
 *   resized to dw x dh as cv2.resize(INTER_LINEAR) does on bytes: coefficients rint((1 - f) 2048) and rint(f 2048) (half to even),
 *   R = S[s] a0 + S[s + 1] a1 along x in int32, out = (((b0 (R0 >> 4)) >> 16) + ((b1 (R1 >> 4)) >> 16) + 2) >> 2 along y.
 * og_resize_f32: src [batch][H][W] float -> dst [batch][h][w].  nearest = 0: the same taps with the float coefficients 1 - f and f,
 *   S[s] a0 + S[s + 1] a1 then R0 b0 + R1 b1, products and sums rounded separately; nearest = 1: s = min(floor(d scale), src - 1) in double.
 * og_megadepth_pairs: `frames` table entries (both images of every pair), each resized to resize_w x resize_h and cut to the tw x th window
 *   at (x0, y0) -> images [frames][th][tw] = resize_linear_u8(grey(image)) / 255.f with grey(R, G, B) = (9798 R + 19235 G + 3735 B + 16384)
 *   >> 15 taken on the source taps (C = 1: the byte), depths [frames][th][tw] = resize_f32(depth), K_out [frames][3][3] =
 *   diag((float)((double)resize_w / W), (float)((double)resize_h / H), 1) K in float, then K[0][2] -= x0, K[1][2] -= y0.  Two launches;
 *   neither the grey image nor a whole resized image or map is written anywhere.
 * og_megadepth_features: `images` table entries -> lafs [images][k][2][3], scores [images][k], descriptors [images][k][desc_dim], depth
 *   [images][k], K_out [images][3][3] with k = num_keypoints <= 4096, n <= 8192 keypoints per image.  Keypoints with start <= c < start +
 *   target on the cropped axis survive (c = lafs[i][axis][2]; axis -1: all) and are shifted by start.  At most k survivors: in their
 *   order, zero padded.  More: the k largest keys (keys, or the scores when keys is NULL) in descending order, the lower index first on
 *   ties.  depth = depth_map[ny(int(y') + start_y)][nx(int(x') + start_x)] through the nearest index maps from image_w x image_h to the
 *   map's own size, 0 for a keypoint outside the cropped image.  K as above with orig -> image and the shift on the cropped axis only.
 *   One launch, one workgroup per image. */
typedef struct og_md_frame {
    const uint8_t* image;         /* [H][W][C] */
    const float* depth;           /* [H][W] */
    const float* K;               /* [3][3] */
    int32_t H, W, C;
    int32_t resize_w, resize_h;
    int32_t x0, y0;               /* origin of the crop in the resized image */
    int32_t reserved;
} og_md_frame;

typedef struct og_md_features {
    const float* lafs;            /* [n][2][3] */
    const float* scores;          /* [n] */
    const float* descriptors;     /* [n][desc_dim] */
    const float* keys;            /* [n] or NULL: what the selection ranks */
    const float* depth;           /* [depth_h][depth_w] */
    const float* K;               /* [3][3] */
    int32_t n;
    int32_t image_w, image_h;     /* the size the features were extracted at */
    int32_t orig_w, orig_h;       /* the size K refers to */
    int32_t depth_w, depth_h;
    int32_t axis, start;          /* crop: axis 0 = x, 1 = y, -1 = none (start 0) */
    int32_t reserved;
} og_md_features;

int og_resize_linear_u8(int32_t batch, int32_t H, int32_t W, int32_t C, const uint8_t* src, int32_t dw, int32_t dh, int32_t x0, int32_t y0,
                        int32_t w, int32_t h, uint8_t* dst, void* stream);
int og_resize_f32(int32_t batch, int32_t H, int32_t W, const float* src, int32_t dw, int32_t dh, int32_t nearest, int32_t x0, int32_t y0,
                  int32_t w, int32_t h, float* dst, void* stream);
int og_megadepth_pairs(int32_t frames, int32_t tw, int32_t th, const og_md_frame* table_host, const og_md_frame* table_dev, float* images,
                       float* depths, float* K_out, int32_t depth_nearest, void* stream);
int og_megadepth_features(int32_t images, int32_t tw, int32_t th, int32_t num_keypoints, int32_t desc_dim, const og_md_features* table_host,
                          const og_md_features* table_dev, float* lafs, float* scores, float* descriptors, float* depth, float* K_out,
                          void* stream);

/* ABI v14, additive -- weak_color_aug (csrc/coloraug.hip): the photometric augmentation of the reference's online training step
 * (models/matching_module.py:55-74 augment, utils/augmentations.py: kornia RandomEqualize, RandomSharpness, RandomSolarize,
 * RandomGaussianNoise).  Device pointers only, no host synchronisation, no allocation, three launches; every result is bit-identical from
 * run to run and independent of the batch it is computed in.  tests/coloraug_ref.py is the specification.
 *
 * og_color_aug: src [batch][C][H][W] float (nominally in [0, 1]) -> dst, the same shape; never in place (dst == src: OG_E_INVALID).
 *   flags [batch] int32: bit 0 equalize, bit 1 sharpness, bit 2 solarize, bit 3 noise -- applied in that order, each only where its bit is
 *   set; a sample with no bit set is copied.  scalars [batch][5] float = sharpness factor, solarize threshold, solarize addition, noise
 *   mean, noise std.  seeds [batch] int64 >= 0 (8-byte aligned).  All three tables live on the device and are not read by the host.
 *   float32, every operation rounded on its own, true divisions; clamp(t, 0, 1) = t < 0 ? 0 : t > 1 ? 1 : t (a NaN stays a NaN):
 *     equalize, per plane:  v = x 255;  q = (v 256) / 255;  bin = q >= 255 ? 255 : q >= 0 ? (int)q : 0 (NaN: 0), idx the same of v;
 *       h = histogram of bin, N = H W, step = (N - h[last non-empty bin]) / 255 in integers;  step == 0: y = v / 255;  else
 *       y = (float)min(255, (sum_{j < idx} h[j] + step / 2) / step) / 255.
 *     sharpness, pixels with 0 < x < W - 1 and 0 < y < H - 1 (the others keep the input):  blur = clamp of the nine taps summed in
 *       row-major order, weights (float)(1 / 13) and, at the centre, (float)(5 / 13);  factor 0: blur;  factor 1: the input;  else
 *       blur + (in - blur) factor, clamped unless 0 < factor < 1.
 *     solarize:  t = clamp(x + addition, 0, 1);  t < threshold ? t : 1 - t.
 *     noise:  i = (c H + y) W + x;  h = mix64(mix64(seed) + i) with mix64(z): z += 0x9E3779B97F4A7C15, z = (z ^ z >> 30) 0xBF58476D1CE4E5B9,
 *       z = (z ^ z >> 27) 0x94D049BB133111EB, z ^ z >> 31 (uint64, wrapping);  u1 = ((h >> 40) + 1) 2^-24, u2 = ((h >> 16) & 0xFFFFFF) 2^-24;
 *       z = sqrtf(-2 logf(u1)) cosf(6.2831855f u2);  out = x + (mean + std z), not clamped.
 *   workspace_dev: og_color_aug_workspace_bytes(batch, C, H, W) bytes, 4-byte aligned, contents irrelevant on entry.
 *   Limits: 1 <= batch <= 65535, 1 <= H, W <= 32768, C in {1, 3}, workspace_bytes large enough, else OG_E_SHAPE; a null pointer
 *   OG_E_INVALID; a table, image or workspace not 4-byte aligned (seeds: 8) OG_E_ALIGN -- all before anything is launched.
 * og_color_aug_workspace_bytes: 0 for a shape og_color_aug refuses. */
size_t og_color_aug_workspace_bytes(int32_t batch, int32_t C, int32_t H, int32_t W);
int og_color_aug(int32_t batch, int32_t C, int32_t H, int32_t W, const float* src, float* dst, const int32_t* flags, const float* scalars,
                 const int64_t* seeds, void* workspace_dev, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* OPENGLUE_AMD_H */
