// The fragment-major weight layout that the fp32 MFMA convolutions (v_mfma_f32_32x32x2_f32) of superpoint.hip and patchnet.hip read:
// one host-side packer for both.  Internal, not part of the ABI.  Everything lives in the unnamed namespace of the including unit.
#pragma once
#include "og_common.h"

namespace {

// Fragment-major weights of a [rows][K] matrix (K a multiple of 8), one coalesced 1 KiB read per 32-row tile and step:
// [jt][step][lane][4] with lane l holding W[32 jt + (l & 31)][8 step + 4 (l >> 5) + e].  value(co, k) gives the folded weight as a
// double, put(offset, double) stores it (and checks that it is finite); rows in [rows, rows_padded) are written as zeros.
template <class Put, class Value>
void pack_fragments(Put put, int64_t dst, int rows, int rows_padded, int K, Value value) {
    for (int co = 0; co < rows_padded; ++co)
        for (int k = 0; k < K; ++k) {
            const int s = k / 8, h = (k % 8) / 4, e = k % 4;
            put(dst + (((int64_t)(co / 32) * (K / 8) + s) * 64 + (co & 31) + 32 * h) * 4 + e, co < rows ? (double)value(co, k) : 0.0);
        }
}

// k of a 3x3 layer whose kernel stages kc input channels per pass: step = (chunk * 9 + tap) * (kc / 8) + kk, and k % 8 runs over
// the step's channels, so ci = kc chunk + 8 kk + k % 8.
inline void conv3x3_k(int k, int kc, int& ci, int& tap) {
    const int s = k / 8, spc = 9 * (kc / 8);
    tap = (s % spc) / (kc / 8);
    ci = (s / spc) * kc + (s % (kc / 8)) * 8 + k % 8;
}

}  // namespace
