// bounded_kernels.hpp - the all-matches and matching-lines scans that keep only whole-word / whole-line occurrences
// (include/sliceslice_hip_bounded.h has the rule; libsliceslice_hip_bounded.so only: scan_inst_bounded.hip instantiates the
// case-sensitive kernels, scan_inst_bounded_nocase.hip the folding ones, ss_bounded.hip is the host side).
//
// Both are their models' text (scan_all_body, SS_LINES_SCAN_KERNEL_AS) with scan_tiles<..., BOUND = true>: a lane's match mask goes
// through bounded_matches right behind the verification that produced it, exact_verify_piece_all's (bits 16..31: offsets handed
// over from the next lane) and verify_flags_all's alike.  Nothing in front of the mask changes - filter bytes, second level, the
// no-match path - and nothing behind it: counts, prefix sums, line bookkeeping and the capacity rules take the mask they are given.
// Only lanes with a confirmed occurrence enter the test; a wave without one executes nothing new.
//
// The mode word `bound` is one more kernel argument, wave-uniform: kBoundWord | kBoundDelim | delimiter << kBoundDelimShift
// (bounded_launch.hpp, which the host side includes too).
//   kBoundWord    a neighbour that is no word byte qualifies ([0-9A-Za-z_] are the word bytes; bytes >= 0x80 are none)
//   kBoundDelim   a neighbour equal to the delimiter qualifies (the line forms: WORD sets both, LINE this one alone)
// An absent neighbour - index -1, index len - always qualifies, and absence is decided from the view's bounds alone: va.end + va.n
// - 1 is the view's length, and no byte outside [0, len) is ever read.  The neighbours are read RAW from memory, also by the folding
// kernels: the word class is the same for a letter and its fold, and the delimiter is never folded.
#pragma once
#include "bounded_launch.hpp"
#include "lines_scan_body.hpp"

namespace ss {

__device__ __forceinline__ bool is_word_byte(uint32_t b)
{
    return ((b | 0x20u) - 'a') < 26u || (b - '0') < 10u || b == '_';
}

// mk: bit t set <=> the needle occurs at hay index i0 + t (t < 32; only offsets below va.end are set).  Returns the bits whose
// occurrence has two qualifying neighbours.
__device__ __forceinline__ uint32_t bounded_matches(uint32_t mk, uint64_t i0, const VerifyArgs &va, uint32_t bound)
{
    const bool word = (bound & kBoundWord) != 0, delim_ok = (bound & kBoundDelim) != 0;       // wave-uniform
    const uint32_t delim = (bound >> kBoundDelimShift) & 0xFFu;
    const uint64_t last = va.end - 1;                   // the one offset whose occurrence ends with the view
    auto qualifies = [&](uint32_t b) { return (word && !is_word_byte(b)) || (delim_ok && b == delim); };
    uint32_t keep = 0;
    while (mk != 0) {
        const int t = __ffs((int)mk) - 1;
        mk &= mk - 1;
        const uint64_t i = i0 + (uint64_t)t;
        // both bytes are asked for before either is looked at: one memory round trip per occurrence
        const uint32_t left = i != 0 ? va.hay[i - 1] : 0u, right = i != last ? va.hay[i + va.n] : 0u;
        if ((i == 0 || qualifies(left)) && (i == last || qualifies(right))) keep |= 1u << t;
    }
    return keep;
}

template <int Q, int MODE, bool ONE_BYTE, bool FOLD>
__global__ void __launch_bounds__(kMaxBlock) scan_all_bounded_kernel(const Problem pr, AllArgs aa, uint64_t tiles_per_block, uint32_t bound)
{
    scan_all_body<Q, MODE, ONE_BYTE, FOLD, true>(pr, aa, tiles_per_block, bound);
}

#define SS_BOUND_PARAM , uint32_t bound
SS_LINES_SCAN_KERNEL_AS(lines_scan_bounded_kernel, false, true, SS_BOUND_PARAM, bound)
SS_LINES_SCAN_KERNEL_AS(lines_scan_bounded_nocase_kernel, true, true, SS_BOUND_PARAM, bound)
#undef SS_BOUND_PARAM

}  // namespace ss
