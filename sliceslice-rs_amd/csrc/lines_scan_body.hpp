// lines_scan_body.hpp - lines_scan_kernel (lines_kernels.hpp has the overview) as a macro, apart from the kernels around it so that its
// case-folding twin (nocase_kernels.hpp, another translation unit) is the same text with scan_tiles' FOLD switch on.
//
// A macro and not a __device__ function that both kernels call: compiled through a function, lines_scan_kernel<0, 0, true> came out
// with one more spilled scalar register than it has (the body is optimised once as a function before it is inlined); expanded in
// place the kernel is token for token what it was.
//
// SS_LINES_SCAN_KERNEL_AS is the text; BOUND, BOUND_PARAM and BOUND_VALUE are scan_tiles' neighbour test, the kernel argument that
// carries its wave-uniform mode word and that argument's name (bounded_kernels.hpp) - off, empty and 0 for SS_LINES_SCAN_KERNEL.
#pragma once
#include "lines_launch.hpp"

// Contiguous tiles per workgroup (1 <= tiles_per_block <= kLineTilesPerBlock), so that workgroup order is address order.
#define SS_LINES_SCAN_KERNEL_AS(NAME, FOLD, BOUND, BOUND_PARAM, BOUND_VALUE)                                                                   \
template <int Q, int MODE, bool ONE_BYTE>                                                                                                      \
__global__ void __launch_bounds__(kMaxBlock) NAME(const Problem pr, LineArgs la, uint64_t tiles_per_block BOUND_PARAM)                         \
{                                                                                                                                              \
    extern __shared__ __attribute__((aligned(16))) uint8_t s_needle[];                                                                         \
    __shared__ uint64_t s_last[kLineTilesPerBlock * kMaxWavesPerBlock];                                                                        \
    __shared__ uint32_t s_flags[kLineTilesPerBlock * kMaxWavesPerBlock];                                                                       \
    __shared__ uint32_t s_nd[kMaxWavesPerBlock], s_cl[kMaxWavesPerBlock];                                                                      \
    constexpr int U = 4;                                                                                                                       \
    const int lane = threadIdx.x & (kWave - 1);                                                                                                \
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);                                                                      \
    const int wpb = (int)(blockDim.x / kWave);                                                                                                 \
    const unsigned tile_shift = (unsigned)__builtin_ctz(blockDim.x / kWave) + (unsigned)__builtin_ctz(U);                                      \
    const uint64_t ntiles = (pr.npieces + ((uint64_t)1 << tile_shift) - 1) >> tile_shift;                                                      \
    const uint64_t t0 = (uint64_t)blockIdx.x * tiles_per_block;                                                                                \
    const uint64_t t1 = t0 + tiles_per_block < ntiles ? t0 + tiles_per_block : ntiles;                                                         \
    LineTiles lt;                                                                                                                              \
    lt.delim_x4 = la.delim * 0x01010101u;                                                                                                      \
    lt.dlo = la.dlo;                                                                                                                           \
    lt.dhi = la.dhi;                                                                                                                           \
    lt.hshift = la.hshift;                                                                                                                     \
    lt.emit = la.mode == kLinesEmit;                                                                                                           \
    lt.tile0 = t0;                                                                                                                             \
    lt.lane_ndelim = lt.lane_closed = 0;                                                                                                       \
    lt.s_last = s_last;                                                                                                                        \
    lt.s_flags = s_flags;                                                                                                                      \
    lt.s_nd = s_nd;                                                                                                                            \
    lt.s_cl = s_cl;                                                                                                                            \
    lt.at = LinePre{0, 0, 0, 0, 0};                                                                                                            \
    lt.begin = la.begin;                                                                                                                       \
    lt.end = la.end;                                                                                                                           \
    lt.number = la.number;                                                                                                                     \
    lt.capacity = la.capacity;                                                                                                                 \
    if (la.mode == kLinesEmit) {                                                                                                               \
        const LinePre *p = la.pre + la.part0 + blockIdx.x;                                                                                     \
        lt.at.ndelim = uniform64(p->ndelim);                                                                                                   \
        lt.at.rank = uniform64(p->rank);                                                                                                       \
        lt.at.last = uniform64(p->last);                                                                                                       \
        lt.at.carry = (uint32_t)__builtin_amdgcn_readfirstlane((int)p->carry);                                                                 \
        const uint32_t closes = (uint32_t)__builtin_amdgcn_readfirstlane((int)p->closes);                                                      \
        if (closes == 0 || lt.at.rank >= la.capacity) return;                                                                                  \
    }                                                                                                                                          \
    scan_tiles<Q, MODE, ONE_BYTE, U, 1, false, false, false, ColdInKernarg, true, true, FOLD, BOUND>(pr, ColdInKernarg{}, s_needle, t0, 1, t1, &lt,\
                                                                                                     nullptr, BOUND_VALUE);                    \
    if (la.mode == kLinesEmit) return;                                                                                                         \
    const uint32_t wn = wave_sum(lt.lane_ndelim), wc = wave_sum(lt.lane_closed);                                                               \
    if (lane == 0) {                                                                                                                           \
        s_nd[wave] = wn;                                                                                                                       \
        s_cl[wave] = wc;                                                                                                                       \
    }                                                                                                                                          \
    __syncthreads();                                                                                                                           \
    if (threadIdx.x == 0) {                                                                                                                    \
        /* the wave summaries in address order: tile by tile, wave by wave */                                                                  \
        LineSum sum = {0, 0, 0, 0, 0};                                                                                                         \
        for (int w = 0; w < wpb; ++w) {                                                                                                        \
            sum.ndelim += s_nd[w];                                                                                                             \
            sum.closed += s_cl[w];                                                                                                             \
        }                                                                                                                                      \
        uint32_t f = 0;                                                                                                                        \
        uint64_t joins = 0, firsts = 0;                                                                                                        \
        for (uint64_t t = 0; t < t1 - t0; ++t) {                                                                                               \
            for (int w = 0; w < wpb; ++w) {                                                                                                    \
                const uint32_t slot = (uint32_t)t * kMaxWavesPerBlock + (uint32_t)w;                                                           \
                const uint32_t e = s_flags[slot];                                                                                              \
                if ((e & kLineHas) == 0) {                                                                                                     \
                    if (e & kLineHead) f |= (f & kLineHas) ? kLineTail : (kLineHead | kLineTail);                                              \
                    continue;                                                                                                                  \
                }                                                                                                                              \
                /* (the wave counted its first delimiter's line when its own head matched: whether that line matches is decided here) */       \
                if (e & kLineHead) ++firsts;                                                                                                   \
                if (f & kLineHas) {                                                                                                            \
                    if ((f & kLineTail) | (e & kLineHead)) ++joins;                                                                            \
                    f = kLineHas | (f & kLineHead) | (e & kLineTail);                                                                          \
                } else {                                                                                                                       \
                    f = kLineHas | ((f | e) & kLineHead) | (e & kLineTail);                                                                    \
                }                                                                                                                              \
                sum.last = s_last[slot];                                                                                                       \
            }                                                                                                                                  \
        }                                                                                                                                      \
        sum.closed = sum.closed + joins - firsts;                                                                                              \
        sum.flags = f;                                                                                                                         \
        la.sum[la.part0 + blockIdx.x] = sum;                                                                                                   \
    }                                                                                                                                          \
}
// the two scans without the neighbour test: no further kernel argument
#define SS_LINES_SCAN_KERNEL(NAME, FOLD) SS_LINES_SCAN_KERNEL_AS(NAME, FOLD, false, , 0u)
