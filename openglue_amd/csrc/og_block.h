// Workgroup-wide helpers for kernels launched with 256 threads (4 waves): a fixed-order sum, an in-place exclusive scan and the
// rank of a flagged thread.  Internal, not part of the ABI.  Everything lives in the unnamed namespace of the including unit.
#pragma once
#include "og_common.h"

namespace {

// Every thread gets the sum over the workgroup: lanes by butterfly, then the four wave sums in wave order -- the same bits from
// run to run.  red: 4 values of LDS; the leading barrier lets consecutive calls share it.
template <class T>
__device__ __forceinline__ T block_sum(T v, T* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) red[wave] = v;
    __syncthreads();
    return ((red[0] + red[1]) + red[2]) + red[3];
}

// Exclusive scan of a[0 .. n) in place by ONE workgroup, the total to *total_out: thread t owns ceil(n / 256) consecutive entries,
// thread 0 scans the 256 partial sums.  The entries are counts (>= 0).  The sums are kept in 64 bits and every offset and the total
// are clamped to INT32_MAX: below 2^31 the results are the plain sums, above it they saturate instead of wrapping, so an offset
// is never negative and a total that does not fit is still larger than any capacity the callers compare it with.
__device__ inline void block_exclusive_scan_inplace(int32_t* __restrict__ a, int n, int32_t* __restrict__ total_out) {
    __shared__ int64_t part[256];
    constexpr int64_t SAT = 2147483647ll;
    const int tid = threadIdx.x;
    const int per = (n + 255) / 256;
    const int lo = min(tid * per, n), hi = min(lo + per, n);
    int64_t sum = 0;
    for (int i = lo; i < hi; ++i) sum += a[i];
    part[tid] = sum;
    __syncthreads();
    if (tid == 0) {
        int64_t run = 0;
        for (int i = 0; i < 256; ++i) {
            const int64_t v = part[i];
            part[i] = run;
            run += v;
        }
        *total_out = (int32_t)(run < SAT ? run : SAT);
    }
    __syncthreads();
    int64_t run = part[tid];
    for (int i = lo; i < hi; ++i) {
        const int64_t v = a[i];
        a[i] = (int32_t)(run < SAT ? run : SAT);
        run += v;
    }
}

// Order-preserving compaction: the number of flagged threads before this one in the workgroup; total = the workgroup's count.
// wsum: 4 ints of LDS.  One barrier inside; a caller that comes back with the same wsum puts its own barrier in between.
__device__ __forceinline__ int block_rank_of(bool flag, int* wsum, int& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long bal = __ballot(flag);
    if (lane == 0) wsum[wave] = __popcll(bal);
    __syncthreads();
    int rank = __popcll(bal & ((1ull << lane) - 1ull));
    for (int w = 0; w < wave; ++w) rank += wsum[w];
    total = wsum[0] + wsum[1] + wsum[2] + wsum[3];
    return rank;
}

}  // namespace
