// bounded_launch.hpp - host-side entry points of the whole-word / whole-line scans (bounded_kernels.hpp; the case-sensitive ones
// are defined in scan_inst_bounded.hip, the folding ones in scan_inst_bounded_nocase.hip; used by ss_bounded.hip).  Same arguments,
// kernel choice (scan_choice.hpp) and return value as launch_scan_all / launch_scan_lines; `bound` is the kernels' mode word.
#pragma once
#include "lines_launch.hpp"
#include "matches_launch.hpp"

namespace ss {

// The mode word, host and kernels alike: kBoundWord - a neighbour that is no word byte qualifies; kBoundDelim - a neighbour equal
// to the delimiter qualifies, and the delimiter sits in the byte at kBoundDelimShift (bounded_kernels.hpp has the rule).
constexpr uint32_t kBoundWord = 1u, kBoundDelim = 2u, kBoundDelimShift = 8u;

bool launch_scan_all_bounded(const Problem &pr, int q, int mode, bool one_byte, const Shape &sh, hipStream_t st, const AllArgs &aa, uint32_t bound);
bool launch_scan_lines_bounded(const Problem &pr, int q, int mode, bool one_byte, const Shape &sh, hipStream_t st, const LineArgs &la, uint32_t bound);
bool launch_scan_all_bounded_nocase(const Problem &pr, int q, int mode, bool one_byte, const Shape &sh, hipStream_t st, const AllArgs &aa, uint32_t bound);
bool launch_scan_lines_bounded_nocase(const Problem &pr, int q, int mode, bool one_byte, const Shape &sh, hipStream_t st, const LineArgs &la, uint32_t bound);

}  // namespace ss
