// inverted_launch.hpp - host-side entry points of the inverted matching-lines kernels (inverted_kernels.hpp; the case-sensitive
// emit launch and the small kernels are defined in scan_inst_inverted.hip, the folding emit launch in scan_inst_inverted_nocase.hip;
// used by ss_inverted.hip, which hands them to the lines host code as a LinesInverted: lines_host.hpp).
#pragma once
#include "bounded_launch.hpp"

namespace ss {

// The emit launch of an inverted call, of ScanLinesFn's type: the grid, kernel choice (scan_choice.hpp) and return value of the sum
// launch in front of it.  la.mode is kLinesEmit, la.sum and la.pre are both read; `bound` == 0 selects the kernels without the
// neighbour test, anything else (a line form's mode word always holds kBoundDelim) those with it.
bool launch_emit_lines_inverted(const Problem &pr, int q, int mode, bool one_byte, const Shape &sh, hipStream_t st, const LineArgs &la, uint32_t bound);
bool launch_emit_lines_inverted_nocase(const Problem &pr, int q, int mode, bool one_byte, const Shape &sh, hipStream_t st, const LineArgs &la, uint32_t bound);
// lines_plain_inverted_kernel over an edge part (emit only; the grid of launch_lines_plain)
hipError_t launch_lines_plain_inverted(const PlainArgs &pa, hipStream_t st);
// lines_total_inverted_kernel: behind launch_lines_combine over the same summaries, with ca.pre the states it wrote
hipError_t launch_lines_total_inverted(const CombineArgs &ca, hipStream_t st);

}  // namespace ss
