// inverted_kernels.hpp - the kernels of the inverted matching-lines calls (include/sliceslice_hip_inverted.h;
// libsliceslice_hip_inverted.so only: scan_inst_inverted.hip and scan_inst_inverted_nocase.hip instantiate them, ss_inverted.hip is
// the host side).
//
// An inverted call runs its model's SUM pass as it is - lines_plain_kernel over the edges, the scan launcher that `how` selects,
// lines_chunk_kernel, lines_combine_kernel - so that every part has its LineSum and, behind the combine, the model's LinePre in
// front of it.  What is new is everything that turns those into the lines WITHOUT a match:
//   lines_total_inverted_kernel   one thread behind the combine: the state behind the last chunk gives the total,
//                                 delimiters - matching lines, and the record of an unterminated last line that holds no match.
//   lines_emit_inverted_kernel    the scan again, EMIT ONLY (scan_tiles<..., INVERT = true>: lines_tiles.hpp complements the
//                                 selection): the mode is a constant, so the summing half of lines_scan_kernel, its epilogue and
//                                 its per-tile LDS entries are not compiled in.  One kernel per (Q, MODE, one-byte) choice of
//                                 scan_choice.hpp x FOLD x BOUND.
//   lines_plain_inverted_kernel   the two edge parts, emit only.  They hold no match, so every delimiter closes a selected line
//                                 except the part's first one when a match is pending in front of it.  Unlike the model's, the
//                                 HEAD part emits too.
// The inverted states are not stored: an emit kernel reads the model's LinePre (rank = matching lines so far, closes = matching
// lines the part closes, saturated at 2^32 - 1) and the part's LineSum.ndelim next to it.  Its first record goes to rank
// pre.ndelim - pre.rank, and it has nothing to do when that is not below the capacity or when sum.ndelim == closes; a saturated
// `closes` says nothing about the difference and skips nothing.
#pragma once
#include "bounded_kernels.hpp"
#include "inverted_launch.hpp"

namespace ss {

// Contiguous tiles per workgroup, as in the sum launch in front of it (SS_LINES_SCAN_KERNEL_AS has the text this is the emit half of).
template <int Q, int MODE, bool ONE_BYTE, bool FOLD, bool BOUND>
__global__ void __launch_bounds__(kMaxBlock) lines_emit_inverted_kernel(const Problem pr, LineArgs la, uint64_t tiles_per_block, uint32_t bound)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t s_needle[];
    __shared__ uint64_t s_last[kMaxWavesPerBlock];
    __shared__ uint32_t s_flags[kMaxWavesPerBlock], s_nd[kMaxWavesPerBlock], s_cl[kMaxWavesPerBlock];
    constexpr int U = 4;
    const unsigned tile_shift = (unsigned)__builtin_ctz(blockDim.x / kWave) + (unsigned)__builtin_ctz(U);
    const uint64_t ntiles = (pr.npieces + ((uint64_t)1 << tile_shift) - 1) >> tile_shift;
    const uint64_t t0 = (uint64_t)blockIdx.x * tiles_per_block;
    const uint64_t t1 = t0 + tiles_per_block < ntiles ? t0 + tiles_per_block : ntiles;
    LineTiles lt;
    lt.delim_x4 = la.delim * 0x01010101u;
    lt.dlo = la.dlo;
    lt.dhi = la.dhi;
    lt.hshift = la.hshift;
    lt.emit = true;
    lt.tile0 = t0;
    lt.lane_ndelim = lt.lane_closed = 0;
    lt.s_last = s_last;
    lt.s_flags = s_flags;
    lt.s_nd = s_nd;
    lt.s_cl = s_cl;
    lt.begin = la.begin;
    lt.end = la.end;
    lt.number = la.number;
    lt.capacity = la.capacity;
    const LinePre *p = la.pre + la.part0 + blockIdx.x;
    lt.at.ndelim = uniform64(p->ndelim);
    lt.at.rank = uniform64(p->rank);
    lt.at.last = uniform64(p->last);
    lt.at.carry = (uint32_t)__builtin_amdgcn_readfirstlane((int)p->carry);
    lt.at.closes = 0;
    const uint32_t closes = (uint32_t)__builtin_amdgcn_readfirstlane((int)p->closes);
    const uint64_t ndelim = uniform64(la.sum[la.part0 + blockIdx.x].ndelim);
    if ((closes != 0xFFFFFFFFu && ndelim == closes) || lt.at.ndelim - lt.at.rank >= la.capacity) return;      // (workgroup-uniform)
    scan_tiles<Q, MODE, ONE_BYTE, U, 1, false, false, false, ColdInKernarg, true, true, FOLD, BOUND, true>(pr, ColdInKernarg{}, s_needle, t0, 1, t1, &lt,
                                                                                                           nullptr, bound);
}

}  // namespace ss
