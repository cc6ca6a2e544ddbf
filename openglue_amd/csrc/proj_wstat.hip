// proj_wstat_kernel -- the q | k | v projections of a 256-d BATCH (launches of more than 8192 token rows), weights stationary, tokens
// streaming.
//
// The tile GEMM these launches ran on (gemm_f16x3.hip: big2, 256 x 256 tiles) streams the weight tile through LDS again for every tile
// and finishes all accumulators of a tile at once: at K = 256 a workgroup is a short burst of operand DMA followed by a 256 KB burst of
// stores, and all CUs run those bursts in step.  Here
//   * a workgroup (512 threads, one per CU) owns ONE slab of 256 output columns -- exactly q, k or v -- for a run of 32-token blocks
//     (og_proj_deal.h); wave w owns columns [32 w, 32 w + 32) of the slab;
//   * a wave's weight slice, 32 columns x 256 k x (hi, lo), is loaded ONCE as A fragments of v_mfma_f32_32x32x16_f16 (16 k-steps x 2 x 4
//     = 128 VGPRs) from the fragment-major stream og_pack_proj_stream writes (one coalesced 1 KiB piece per load) and stays in registers:
//     no weight traffic through LDS;
//   * the token blocks (32 hl32 rows of x = 32 KB) come through a 3-slot LDS ring by LDS-DMA, two blocks ahead, counted vmcnt, one
//     barrier per block; every wave reads the same B fragments from it (32 ds_read_b128 for 48 MFMAs);
//   * a wave finishes one 32 x 32 tile per block and writes it -- scaled, split to (hi, lo), transposed through its own 4 KB LDS slab --
//     under the MFMAs of the NEXT block (two accumulators), so a workgroup never holds more than 4 KB per wave of unwritten output and
//     the chip sees reads, matrix work and writes interleaved for the whole life of the launch.
// Arithmetic: as big2 (accumulator = bias / scale; k-steps ascending; per k-step Wl xh, Wh xl, Wh xh; times scale; og_split4): the
// planes are bit-identical to that kernel's.  No communication between workgroups.
#include <type_traits>

#include "og_common.h"
#include "og_proj_deal.h"

namespace {

typedef __attribute__((address_space(3))) void og_lds_void;
typedef __attribute__((address_space(1))) const void og_glb_void;

// Compile-time ablations (experiment builds; results are wrong by construction): 1 = no global stores, 2 = no MFMA, 4 = no fragment reads
// after the first of a block, 8 = no LDS-DMA after the first two blocks, 16 = no epilogue at all.
#ifndef OG_WSTAT_ABL
#define OG_WSTAT_ABL 0
#endif

constexpr int WS_G = 256;                 // workgroups of a launch: one per CU
constexpr int WS_BLK = 32;                // tokens of a block
constexpr int WS_SLOT = 8 * 32 * 128;     // one block in LDS: 8 k-groups x 32 rows x 128 B (hi 64 B | lo 64 B of 32 channels)
constexpr int WS_RING = 3 * WS_SLOT;
constexpr int WS_SLAB = 2 * 32 * 64;      // per-wave epilogue slab: 2 planes x 32 tokens x 64 B

struct ProjWstatArgs {
    const _Float16* X; int64_t ld; int M;      // [M] hl32 rows, the first 512 halves = x
    const char* wstream;                       // og_pack_proj_stream, K = 256
    const float* bias;                         // [N]
    const float* scale_dev;                    // DEVICE: 1 / pre-scale of the matrix
    _Float16* Ch; _Float16* Cl; int64_t ldc;   // output planes [M][ldc]
    int sa0, sb0;                              // first slab (256 columns) of row range A / B
    OgProjDeal deal;
};

__global__ __launch_bounds__(512) void proj_wstat_kernel(ProjWstatArgs g) {
    __shared__ __attribute__((aligned(16))) char smem[WS_RING + 8 * WS_SLAB];
    static_assert(WS_RING + 8 * WS_SLAB == 128 * 1024 && WS_BLK == 32, "LDS budget; og_proj_deal_rows counts 32-token blocks");
    int range, slabi, blk0, blk1;
    if (!og_proj_deal_unit(g.deal, og_proj_deal_slot(blockIdx.x, WS_G), range, slabi, blk0, blk1)) return;
    const int slab = (range ? g.sb0 : g.sa0) + slabi;
    const int cnt = blk1 - blk0;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31, hi = lane >> 5;
    const unsigned lds0 = (unsigned)(uintptr_t)(__attribute__((address_space(3))) char*)smem;

    // ---- token blocks: wave w fetches k-group w (one 128-byte line per row) of the 32 rows, 8 rows per DMA piece; 16-byte chunk c of
    //      row r lands at chunk c ^ ((r >> 1) & 7) (swizzle on the source address, matched by the fragment reads).
    //      Addressing (as the attention tile loop): a SCALAR block base + four loop-invariant 32-bit lane offsets, the four
    //      pieces in ONE asm block with one M0 write.  The instruction offset h KiB moves the LDS AND the global address, so the lane
    //      offset of piece h takes it back out and the base sits 3 KiB low to keep every lane offset non-negative.  The blocks of a run
    //      are issued in order: the base advances by a scalar add of 32 rows per issue.  Rows past M are clamped (computed, never
    //      stored): only the run's LAST block can hold such rows, it has its own offsets (xoffc: equal to xoff when that block is whole) ----
    const int64_t ldb = g.ld * 2;
    unsigned xoff[4], xoffc[4];
    {
        const int lastrt = g.M - 1 - (blk1 - 1) * WS_BLK;
#pragma unroll
        for (int h = 0; h < 4; ++h) {
            const int rt = h * 8 + (lane >> 3);
            const unsigned ch = (unsigned)((((lane & 7) ^ ((rt >> 1) & 7)) << 4) + (3 - h) * 1024);
            xoff[h] = (unsigned)(rt * (int)ldb) + ch;
            xoffc[h] = (unsigned)((rt < lastrt ? rt : lastrt) * (int)ldb) + ch;
            asm volatile("" : "+v"(xoff[h]), "+v"(xoffc[h]));
        }
    }
    const char* xsrc = reinterpret_cast<const char*>(g.X) + wave * 128 + (int64_t)blk0 * WS_BLK * ldb - 3072;      // the next block to issue; uniform
    const int64_t xstep = WS_BLK * ldb;
    const unsigned m0_wave = lds0 + (unsigned)(wave * 4096);
    auto issue_pieces = [&](const unsigned (&o)[4], int slot) {
        const unsigned m0v = m0_wave + (unsigned)(slot * WS_SLOT);
        asm volatile("s_mov_b32 m0, %5\n\t"
                     "s_nop 0\n\t"
                     "global_load_lds_dwordx4 %0, %4\n\t"
                     "global_load_lds_dwordx4 %1, %4 offset:1024\n\t"
                     "global_load_lds_dwordx4 %2, %4 offset:2048\n\t"
                     "global_load_lds_dwordx4 %3, %4 offset:3072"
                     :: "v"(o[0]), "v"(o[1]), "v"(o[2]), "v"(o[3]), "s"(xsrc), "s"(m0v) : "memory");
        xsrc += xstep;
    };
    // block n of the run (the blocks are issued in order: xsrc points at it).  STEADY: known not to be the run's last block
    auto issue_block = [&](auto STEADY, int n, int slot) {
        if (decltype(STEADY)::value || n + 1 < cnt) issue_pieces(xoff, slot);
        else issue_pieces(xoffc, slot);
    };
    using Steady = std::integral_constant<bool, true>;
    using Generic = std::integral_constant<bool, false>;
    issue_block(Generic{}, 0, 0);
    if (cnt > 1) issue_block(Generic{}, 1, 1);

    // ---- this wave's weights and bias ----
    const int col0 = slab * 256 + wave * 32;
    f16x8 wh[16], wl[16];
    {
        const char* wsrc = g.wstream + (int64_t)(col0 >> 5) * (16 * 2 * 1024) + lane * 16;
#pragma unroll
        for (int ks = 0; ks < 16; ++ks) {
            wh[ks] = *reinterpret_cast<const f16x8*>(wsrc + (2 * ks) * 1024);
            wl[ks] = *reinterpret_cast<const f16x8*>(wsrc + (2 * ks + 1) * 1024);
        }
    }
    const float sc = g.scale_dev[0];
    f32x16 binit;                                       // register 4 q + e = channel 8 q + 4 hi + e (og_common.h: mfma32_row)
    {
        const float isc = 1.f / sc;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const f32x4 b = *reinterpret_cast<const f32x4*>(g.bias + col0 + 8 * q + 4 * hi) * isc;
#pragma unroll
            for (int e = 0; e < 4; ++e) binit[4 * q + e] = b[e];
        }
    }
#pragma unroll
    for (int ks = 0; ks < 16; ++ks) asm volatile("" : "+v"(wh[ks]), "+v"(wl[ks]));
    asm volatile("" : "+v"(binit));

    // ---- fragment reads: token l31, k-step ks = channels 16 ks + 8 hi .. + 7 of k-group ks >> 1: chunk 2 (ks & 1) + hi, lo = chunk ^ 4 ----
    unsigned xk[2][2];
    {
        const unsigned swz = (unsigned)((l31 >> 1) & 7);
#pragma unroll
        for (int o = 0; o < 2; ++o) {
            xk[o][0] = (unsigned)(l31 * 128) + ((((unsigned)(2 * o + hi)) ^ swz) << 4);
            xk[o][1] = xk[o][0] ^ 64u;
        }
    }
    unsigned xa[2][2];
    f16x8 xh[2], xl[2];
    auto set_x = [&](int slot) {
        const unsigned b = lds0 + (unsigned)(slot * WS_SLOT);
#pragma unroll
        for (int o = 0; o < 2; ++o) { xa[o][0] = b + xk[o][0]; xa[o][1] = b + xk[o][1]; }
    };
    auto lds_read = [&](f16x8& dst, unsigned addr, int imm) { asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(dst) : "v"(addr), "i"(imm)); };
    auto read_x = [&](int ks, int buf) {
        lds_read(xh[buf], xa[ks & 1][0], (ks >> 1) * 4096);
        lds_read(xl[buf], xa[ks & 1][1], (ks >> 1) * 4096);
    };
    auto wait_frag = [&](int buf, int newer) {
        if (newer == 0) asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(xh[buf]), "+v"(xl[buf]));
        else asm volatile("s_waitcnt lgkmcnt(2)" : "+v"(xh[buf]), "+v"(xl[buf]));
    };

    // ---- epilogue of one finished 32 x 32 tile, in four parts that the k-loop of the next block spreads over its MFMAs.  Slab: plane p
    //      at p * 2048, token row r at r * 64, 16-byte chunk c (channels 8 c .. 8 c + 7) at chunk c ^ ((r >> 2) & 3): the accumulator-layout
    //      writes (32 rows at one logical chunk, 8 B per lane) and the row reads (16 rows x 64 B per instruction) are both conflict-free ----
    const unsigned slab0 = lds0 + WS_RING + wave * WS_SLAB;
    unsigned ew[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) ew[q] = slab0 + (unsigned)(l31 * 64 + ((q ^ ((l31 >> 2) & 3)) << 4) + hi * 8);
    const unsigned er = slab0 + (unsigned)((lane >> 2) * 64 + (((lane & 3) ^ ((lane >> 4) & 3)) << 4));
    // Store addressing: two 64-bit plane bases per wave (SGPRs: the tile to store next; tiles are stored in order, the bases advance by a scalar
    // add of 32 rows behind a tile's lo plane) + two loop-invariant lane offsets, rows (lane >> 2) and 16 + (lane >> 2) of the tile.
    const int64_t ldcb = g.ldc * 2;
    unsigned soff[2];
    soff[0] = (unsigned)((lane >> 2) * (int)ldcb + col0 * 2 + (lane & 3) * 16);
    soff[1] = soff[0] + (unsigned)(16 * (int)ldcb);
    asm volatile("" : "+v"(soff[0]), "+v"(soff[1]));
    char* sch = reinterpret_cast<char*>(g.Ch) + (int64_t)blk0 * WS_BLK * ldcb;
    char* scl = reinterpret_cast<char*>(g.Cl) + (int64_t)blk0 * WS_BLK * ldcb;
    const int64_t sstep = WS_BLK * ldcb;
    unsigned ph[4][2], pl[4][2];
    f16x8 tt[2];
    auto epi_split = [&](f32x16& a) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            float v[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) asm volatile("v_mul_f32 %0, %1, %2" : "=v"(v[e]) : "s"(sc), "v"(a[4 * q + e]));      // one rounding, no packed fp32 under the MFMAs
            og_split4(v[0], v[1], v[2], v[3], ph[q][0], pl[q][0], ph[q][1], pl[q][1]);
        }
    };
    auto epi_write = [&]() {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            asm volatile("ds_write_b64 %0, %1" :: "v"(ew[q]), "v"(make_uint2(ph[q][0], ph[q][1])) : "memory");
            asm volatile("ds_write_b64 %0, %1 offset:2048" :: "v"(ew[q]), "v"(make_uint2(pl[q][0], pl[q][1])) : "memory");
        }
    };
    // plane p (0 = hi, 1 = lo) of the slab -> two stores of 16 rows x 64 B.  LDS serves a wave's instructions in order, so the row reads
    // need no wait behind the column writes; the stores wait for the row reads with a COUNTED lgkmcnt (`newer` = LDS operations issued
    // since: the fragment reads of the k-steps in between), so that the epilogue never drains the fragment pipeline.
    auto epi_read = [&](int p) {
#pragma unroll
        for (int i = 0; i < 2; ++i) asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(tt[i]) : "v"(er), "i"(p * 2048 + i * 1024) : "memory");
    };
    // FULL: a whole tile (every tile but the last of a run): no row predicate
    auto epi_store = [&](auto FULL, int p, int newer) {
        if (newer >= 4) asm volatile("s_waitcnt lgkmcnt(4)" : "+v"(tt[0]), "+v"(tt[1]) :: "memory");
        else asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(tt[0]), "+v"(tt[1]) :: "memory");
        char* const base = p ? scl : sch;
        if constexpr (decltype(FULL)::value) {
            if (!(OG_WSTAT_ABL & 1))
                asm volatile("global_store_dwordx4 %0, %2, %4\n\t"
                             "global_store_dwordx4 %1, %3, %4"
                             :: "v"(soff[0]), "v"(soff[1]), "v"(tt[0]), "v"(tt[1]), "s"(base) : "memory");
        } else {
            const int left = g.M - (blk1 - 1) * WS_BLK - (lane >> 2);      // rows of the run's last tile from this lane's first row on
#pragma unroll
            for (int i = 0; i < 2; ++i)
                if (!(OG_WSTAT_ABL & 1) && i * 16 < left) *reinterpret_cast<f16x8*>(base + soff[i]) = tt[i];
        }
        if (p) { sch += sstep; scl += sstep; }
    };

    // everything this wave asked for so far has landed: block 0, block 1, weights, bias
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");

    // Block n.  Vector-memory operations complete in issue order; at the top of block n >= 2 the operations younger than the pieces of
    // block n (issued at the top of block n - 2) are the 4 stores of tile n - 3, the 4 pieces of block n + 1 and the 4 stores of tile n - 2
    // (all of them full tiles: only the last tile of a run can be partial).
    // STEADY (compile time): 3 <= n and n + 2 is not the run's last block -- the wait is vmcnt(12), the pieces of block n + 2 are issued
    // unconditionally with the unclamped offsets, the tile of block n - 1 is written.  The first three and the last (up to four) blocks
    // of a run take the generic form, which asks.
    auto do_block = [&](auto STEADY, f32x16& acc, f32x16& prev, int n, int slot) __attribute__((always_inline)) {
        constexpr bool steady = decltype(STEADY)::value;
        if (steady) asm volatile("s_waitcnt vmcnt(12)" ::: "memory");
        else if (n >= 2) {
            const bool nxt = n + 1 < cnt, old = n >= 3;
            if (nxt && old) asm volatile("s_waitcnt vmcnt(12)" ::: "memory");
            else if (nxt || old) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
            else asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
        }
        __builtin_amdgcn_s_barrier();       // every wave's pieces of block n are in LDS; every wave is past its reads of block n - 1
        if ((steady || n + 2 < cnt) && !(OG_WSTAT_ABL & 8)) issue_block(STEADY, n + 2, slot == 0 ? 2 : slot - 1);      // (n + 2) % 3: the slot of block n - 1
        set_x(slot);
        read_x(0, 0);
        const bool ep = (steady || n > 0) && !(OG_WSTAT_ABL & 16);
#pragma unroll
        for (int ks = 0; ks < 16; ++ks) {
            if (ks < 15 && !(OG_WSTAT_ABL & 4)) read_x(ks + 1, (ks + 1) & 1);
            if (ep) {
                // (each part sits behind the fragment reads of k-step ks + 1; between a plane's row reads and its stores lie the
                //  fragment reads of two more k-steps: 4 newer LDS operations)
                if (ks == 1) epi_split(prev);
                if (ks == 3) epi_write();
                if (ks == 5) epi_read(0);
                if (ks == 7) epi_store(std::true_type{}, 0, 4);
                if (ks == 8) epi_read(1);
                if (ks == 10) epi_store(std::true_type{}, 1, 4);
            }
            wait_frag(ks & 1, ks < 15 ? 2 : 0);
            __builtin_amdgcn_sched_barrier(0);
#if OG_WSTAT_ABL & 2
            if (ks == 0) acc = binit;
            asm volatile("" : "+v"(acc) : "v"(wl[ks]), "v"(wh[ks]), "v"(xh[ks & 1]), "v"(xl[ks & 1]));
#else
            acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(wl[ks], xh[ks & 1], ks == 0 ? binit : acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(wh[ks], xl[ks & 1], acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(wh[ks], xh[ks & 1], acc, 0, 0, 0);
#endif
            __builtin_amdgcn_sched_barrier(0);
        }
    };
    auto next3 = [](int v) { return v == 2 ? 0 : v + 1; };
    f32x16 acc0, acc1;
    // blocks 0, 1, 2 (block n accumulates in acc0 for even n, acc1 for odd n; ring slot n % 3)
    do_block(Generic{}, acc0, acc1, 0, 0);
    if (cnt > 1) do_block(Generic{}, acc1, acc0, 1, 1);
    if (cnt > 2) do_block(Generic{}, acc0, acc1, 2, 2);
    if (cnt > 3) {
        int n = 3, slot = 0;
        // the steady loop: block n + 3 is issued in it, and must not be the run's last
#pragma unroll 1
        for (; n + 4 < cnt; n += 2) {
            do_block(Steady{}, acc1, acc0, n, slot);
            slot = next3(slot);
            do_block(Steady{}, acc0, acc1, n + 1, slot);
            slot = next3(slot);
        }
        // the last one to four blocks
        do_block(Generic{}, acc1, acc0, n, slot);
        if (n + 1 < cnt) {
            slot = next3(slot);
            do_block(Generic{}, acc0, acc1, n + 1, slot);
            if (n + 2 < cnt) {
                slot = next3(slot);
                do_block(Generic{}, acc1, acc0, n + 2, slot);
                if (n + 3 < cnt) do_block(Generic{}, acc0, acc1, n + 3, next3(slot));
            }
        }
    }
    // (the tail reads the accumulator right behind the last MFMA; the hazard recognizer does not look inside inline asm)
    asm volatile("s_nop 15\n\ts_nop 15" ::: "memory");
    if (cnt & 1) epi_split(acc0);
    else epi_split(acc1);
    epi_write();
    epi_read(0);
    epi_store(std::false_type{}, 0, 0);
    epi_read(1);
    epi_store(std::false_type{}, 1, 0);
}

}  // namespace

// One OG_PROJ_WSTAT step (og_launch_proj has checked it): rows [0, s.rows) of X times the 256-column slabs [a0, a1) of the packed matrix for the
// rows below split_row, [b0, b1) for the others (split_row <= 0 or >= rows: every row takes the second / the first range).
int og_launch_proj_wstat(const ProjArgs& a, const OgProjStep& s, hipStream_t stream) {
    ProjWstatArgs g{a.X, a.ld, s.rows, a.wsmall, a.bias, a.scale_dev, a.Ch, a.Cl, a.ldc, s.a0, s.b0, og_proj_deal_rows(s.rows, s.split_row, s.a1 - s.a0, s.b1 - s.b0, WS_G)};
    if (g.deal.ta * g.deal.na + g.deal.tb * g.deal.nb == 0) return 0;       // both ranges empty: nothing to write
    hipLaunchKernelGGL(proj_wstat_kernel, dim3(WS_G), dim3(512), 0, stream, g);
    return og_launch_status();
}
