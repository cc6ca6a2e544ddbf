// The reference's optimizer step (models/matching_module.py:133-147 configure_optimizers: torch.optim.Adam + StepLR stepped every
// iteration; train.py:73 gradient_clip_val = torch.nn.utils.clip_grad_norm_) as three launches whatever the number of parameters:
//
//   adam_gradnorm_kernel   one pass over the flat gradient buffer, float4 loads; workgroup c reduces floats [c kNormChunk, (c+1) kNormChunk):
//                          fp32 squares accumulated in fp64, one fp64 partial per workgroup, no atomics
//   adam_prepare_kernel    one workgroup: the partials summed in a fixed order in fp64 (thread t takes a contiguous index range, the 256
//                          thread sums go through a fixed tree), then the scalars of the step, all in fp64, written with plain stores:
//                          total_norm, clip_coef, step (incremented), lr_t, step_size, 1 / sqrt(bias_correction2)
//   adam_update_kernel     workgroup c = one chunk of one parameter (chunk map): float4 loads of p, g, m, v (scalar tail for numel % 4),
//                          g <- clip_coef g, torch's single-tensor Adam statement for statement, stores of p, m, v and g = 0
//
// Layout (og_adam_layout): the optimizer owns three flat fp32 buffers grad / exp_avg / exp_avg_sq in which parameter i has the segment
// [offset_i, offset_i + numel_i), offset_i a multiple of 4; the padding between segments is zero and is never written.  Parameters stay
// where the caller keeps them: the device table holds {pointer, offset, numel} per parameter, the chunk map {parameter, chunk within
// it} per update workgroup.  The step count lives in the scalars block: a step reads nothing from the host but its kernel arguments.
#include "og_common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kChunk = OG_ADAM_CHUNK;              // floats of one parameter per update workgroup: 4 float4 per thread
constexpr int kNormChunk = OG_ADAM_NORM_CHUNK;     // floats of the flat gradient buffer per norm workgroup: 8 float4 per thread
constexpr int kUpdateVecs = kChunk / 4 / kThreads;
constexpr int kNormVecs = kNormChunk / 4 / kThreads;
static_assert(kUpdateVecs * 4 * kThreads == kChunk && kNormVecs * 4 * kThreads == kNormChunk, "chunks are whole float4 sweeps");

struct AdamTensor {            // one row of the device table (three 8-byte words: the binding writes it as int64[count][3])
    float* param;
    int64_t offset;            // floats, multiple of 4
    int64_t numel;
};
static_assert(sizeof(AdamTensor) == 24, "table row");

// fixed-order sum of one double per thread over the workgroup: xor tree inside the wave, then the 4 wave sums in wave order
__device__ __forceinline__ double block_sum(double v, double* lds) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) lds[wave] = v;
    __syncthreads();
    double s = lds[0];
#pragma unroll
    for (int w = 1; w < kThreads / 64; ++w) s += lds[w];
    return s;
}

__global__ __launch_bounds__(kThreads) void adam_gradnorm_kernel(const float* __restrict__ grad, int64_t total, double* __restrict__ partials) {
    __shared__ double lds[kThreads / 64];
    const int64_t base = (int64_t)blockIdx.x * kNormChunk;
    const int64_t nvec = ((total - base < kNormChunk ? total - base : kNormChunk)) >> 2;      // total is a multiple of 4
    const f32x4* g4 = reinterpret_cast<const f32x4*>(grad + base);
    f32x4 g[kNormVecs];
#pragma unroll
    for (int u = 0; u < kNormVecs; ++u) {
        const int i = u * kThreads + threadIdx.x;
        g[u] = i < nvec ? g4[i] : f32x4{0.f, 0.f, 0.f, 0.f};
    }
    double acc = 0.0;
#pragma unroll
    for (int u = 0; u < kNormVecs; ++u)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float sq = g[u][e] * g[u][e];            // the square is rounded to fp32, the sum is fp64
            acc += (double)sq;
        }
    const double s = block_sum(acc, lds);
    if (threadIdx.x == 0) partials[blockIdx.x] = s;
}

struct AdamHyper { double lr, gamma, beta1, beta2, max_norm; };

__global__ __launch_bounds__(kThreads) void adam_prepare_kernel(const double* __restrict__ partials, int num_partials, int clip, AdamHyper h,
                                                                double* __restrict__ scalars) {
    __shared__ double lds[kThreads / 64];
    double total_norm = __builtin_nan(""), clip_coef = 1.0;
    if (clip) {
        const int per = (num_partials + kThreads - 1) / kThreads;
        const int lo = threadIdx.x * per, hi = lo + per < num_partials ? lo + per : num_partials;
        double acc = 0.0;
        for (int i = lo; i < hi; ++i) acc += partials[i];
        total_norm = sqrt(block_sum(acc, lds));
        const double c = h.max_norm / (total_norm + 1e-6);
        clip_coef = c < 1.0 ? c : 1.0;                 // torch.clamp(max=1.0): a NaN coefficient stays NaN, as under torch
        if (c != c) clip_coef = c;
    }
    if (threadIdx.x == 0) {
        const double step = scalars[OG_ADAM_STEP] + 1.0;
        const double lr_t = h.lr * pow(h.gamma, step - 1.0);
        scalars[OG_ADAM_TOTAL_NORM] = total_norm;
        scalars[OG_ADAM_CLIP_COEF] = clip_coef;
        scalars[OG_ADAM_STEP] = step;
        scalars[OG_ADAM_LR] = lr_t;
        scalars[OG_ADAM_STEP_SIZE] = lr_t / (1.0 - pow(h.beta1, step));
        scalars[OG_ADAM_INV_SQRT_BC2] = 1.0 / sqrt(1.0 - pow(h.beta2, step));
    }
}

struct AdamCoef { float clip, beta1, one_minus_beta1, beta2, one_minus_beta2, step_size, inv_sqrt_bc2, eps; };

// torch/optim/adam.py _single_tensor_adam, one element; every product and sum rounded on its own, as the separate torch kernels round them
__device__ __forceinline__ void adam_element(float& p, float& g, float& m, float& v, const AdamCoef& c) {
#pragma clang fp contract(off)
    g = c.clip * g;                                             // clip_grad_norm_: g.mul_(clip_coef_clamped)
    m = m + c.one_minus_beta1 * (g - m);                        // exp_avg.lerp_(grad, 1 - beta1)
    v = c.beta2 * v + c.one_minus_beta2 * g * g;                // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value=1 - beta2)
    const float denom = sqrtf(v) * c.inv_sqrt_bc2 + c.eps;      // (exp_avg_sq.sqrt() / bias_correction2_sqrt).add_(eps)
    p = p - c.step_size * (m / denom);                          // param.addcdiv_(exp_avg, denom, value=-step_size)
}

__global__ __launch_bounds__(kThreads) void adam_update_kernel(const AdamTensor* __restrict__ table, const int32_t* __restrict__ chunk_map,
                                                               float* __restrict__ grad, float* __restrict__ exp_avg,
                                                               float* __restrict__ exp_avg_sq, const double* __restrict__ scalars,
                                                               float beta1, float one_minus_beta1, float beta2, float one_minus_beta2,
                                                               float eps) {
    const int t = chunk_map[2 * blockIdx.x];
    const int64_t start = (int64_t)chunk_map[2 * blockIdx.x + 1] * kChunk;
    const AdamTensor T = table[t];
    const int64_t left = T.numel - start;
    const int count = (int)(left < kChunk ? left : kChunk);
    const int nvec = count >> 2;
    AdamCoef c;
    c.clip = (float)scalars[OG_ADAM_CLIP_COEF];
    c.beta1 = beta1; c.one_minus_beta1 = one_minus_beta1;
    c.beta2 = beta2; c.one_minus_beta2 = one_minus_beta2;
    c.step_size = (float)scalars[OG_ADAM_STEP_SIZE];
    c.inv_sqrt_bc2 = (float)scalars[OG_ADAM_INV_SQRT_BC2];
    c.eps = eps;
    float* p = T.param + start;                                 // start is a multiple of kChunk: as aligned as the parameter
    float* g = grad + T.offset + start;
    float* m = exp_avg + T.offset + start;
    float* v = exp_avg_sq + T.offset + start;
    f32x4* p4 = reinterpret_cast<f32x4*>(p);
    f32x4* g4 = reinterpret_cast<f32x4*>(g);
    f32x4* m4 = reinterpret_cast<f32x4*>(m);
    f32x4* v4 = reinterpret_cast<f32x4*>(v);
    f32x4 P[kUpdateVecs], G[kUpdateVecs], M[kUpdateVecs], V[kUpdateVecs];
#pragma unroll
    for (int u = 0; u < kUpdateVecs; ++u) {                     // every load of the chunk is issued before the first store
        const int i = u * kThreads + threadIdx.x;
        if (i < nvec) { P[u] = p4[i]; G[u] = g4[i]; M[u] = m4[i]; V[u] = v4[i]; }
    }
#pragma unroll
    for (int u = 0; u < kUpdateVecs; ++u) {
        const int i = u * kThreads + threadIdx.x;
        if (i < nvec) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float pe = P[u][e], ge = G[u][e], me = M[u][e], ve = V[u][e];
                adam_element(pe, ge, me, ve, c);
                P[u][e] = pe; M[u][e] = me; V[u][e] = ve;
            }
            p4[i] = P[u]; m4[i] = M[u]; v4[i] = V[u];
            g4[i] = f32x4{0.f, 0.f, 0.f, 0.f};                  // the next backward accumulates into zeros
        }
    }
    const int i = 4 * nvec + threadIdx.x;                       // numel % 4 elements at the end of the parameter's last chunk
    if (threadIdx.x < 3 && i < count) {
        float pe = p[i], ge = g[i], me = m[i], ve = v[i];
        adam_element(pe, ge, me, ve, c);
        p[i] = pe; m[i] = me; v[i] = ve; g[i] = 0.f;
    }
}

}  // namespace

extern "C" int og_adam_layout(int32_t count, const int64_t* numel, int64_t* offsets, int32_t* chunk_map, og_adam_layout_t* layout) {
    if (count <= 0 || !numel || !layout) return OG_E_INVALID;
    int64_t total = 0, chunks = 0;
    for (int32_t i = 0; i < count; ++i) {
        if (numel[i] <= 0) return OG_E_INVALID;
        if (offsets) offsets[i] = total;
        const int64_t nc = (numel[i] + kChunk - 1) / kChunk;
        if (chunk_map)
            for (int64_t c = 0; c < nc; ++c) {
                chunk_map[2 * (chunks + c)] = i;
                chunk_map[2 * (chunks + c) + 1] = (int32_t)c;
            }
        chunks += nc;
        total += og_round_up(numel[i], 4);
        if (chunks > INT32_MAX || total > ((int64_t)1 << 40)) return OG_E_SHAPE;
    }
    layout->total = total;
    layout->num_chunks = (int32_t)chunks;
    layout->num_partials = (int32_t)((total + kNormChunk - 1) / kNormChunk);
    layout->chunk = kChunk;
    layout->table_bytes = (int64_t)count * (int64_t)sizeof(AdamTensor);
    layout->workspace_bytes = (int64_t)sizeof(double) * (OG_ADAM_SCALARS + layout->num_partials);
    return 0;
}

extern "C" int og_adam_step(int32_t count, const void* const* params, const void* table_dev, const int32_t* chunk_map_dev,
                            int32_t num_chunks, int64_t total, float* grad, float* exp_avg, float* exp_avg_sq, double* workspace_dev,
                            double lr, double gamma, double beta1, double beta2, double eps, int32_t clip, double max_norm,
                            void* stream) {
    og_clear_status();
    if (count <= 0 || num_chunks <= 0 || total <= 0 || (total & 3)) return OG_E_INVALID;
    if (!params || !table_dev || !chunk_map_dev || !grad || !exp_avg || !exp_avg_sq || !workspace_dev) return OG_E_INVALID;
    for (int32_t i = 0; i < count; ++i) {
        if (!params[i]) return OG_E_INVALID;
        if ((uintptr_t)params[i] & 15) return OG_E_ALIGN;
    }
    if (((uintptr_t)grad | (uintptr_t)exp_avg | (uintptr_t)exp_avg_sq) & 15) return OG_E_ALIGN;
    if ((((uintptr_t)workspace_dev | (uintptr_t)table_dev) & 7) || ((uintptr_t)chunk_map_dev & 3)) return OG_E_ALIGN;
    hipStream_t st = (hipStream_t)stream;
    double* scalars = workspace_dev;
    double* partials = workspace_dev + OG_ADAM_SCALARS;
    const int num_partials = (int)((total + kNormChunk - 1) / kNormChunk);
    if (clip) hipLaunchKernelGGL(adam_gradnorm_kernel, dim3(num_partials), dim3(kThreads), 0, st, grad, total, partials);
    const AdamHyper h{lr, gamma, beta1, beta2, max_norm};
    hipLaunchKernelGGL(adam_prepare_kernel, dim3(1), dim3(kThreads), 0, st, partials, num_partials, clip ? 1 : 0, h, scalars);
    hipLaunchKernelGGL(adam_update_kernel, dim3(num_chunks), dim3(kThreads), 0, st, (const AdamTensor*)table_dev, chunk_map_dev, grad,
                       exp_avg, exp_avg_sq, scalars, (float)beta1, (float)(1.0 - beta1), (float)beta2, (float)(1.0 - beta2), (float)eps);   // 1 - beta in fp64 first, as torch's Python scalars
    return og_launch_status();
}
