// scan_inst_bounded.hip - the case-sensitive whole-word / whole-line scans (bounded_kernels.hpp): one scan_all_bounded_kernel and
// one lines_scan_bounded_kernel per (Q, MODE, one-byte) combination their models have - 4 Q x MODE 0, 4 Q x MODE 2, one-byte: 9 each,
// chosen by scan_choice.hpp.  Compiled into libsliceslice_hip_bounded.so only (ss_bounded.hip is the host side); the folding ones
// are scan_inst_bounded_nocase.hip's, so that the two halves compile side by side.
#include "bounded_kernels.hpp"
#include "bounded_launch.hpp"
#include "scan_choice.hpp"

namespace ss {

bool launch_scan_all_bounded(const Problem &pr, int q, int mode, bool one_byte, const Shape &sh, hipStream_t st, const AllArgs &aa, uint32_t bound)
{
    return choose_scan_kernel(q, mode, one_byte, [&](auto Q, auto MODE, auto ONE_BYTE) {
        scan_all_bounded_kernel<decltype(Q)::value, decltype(MODE)::value, decltype(ONE_BYTE)::value, false>
            <<<dim3(sh.blocks), dim3(sh.block), scan_dyn_lds(sh), st>>>(pr, aa, sh.tpb, bound);
    });
}

bool launch_scan_lines_bounded(const Problem &pr, int q, int mode, bool one_byte, const Shape &sh, hipStream_t st, const LineArgs &la, uint32_t bound)
{
    return choose_scan_kernel(q, mode, one_byte, [&](auto Q, auto MODE, auto ONE_BYTE) {
        lines_scan_bounded_kernel<decltype(Q)::value, decltype(MODE)::value, decltype(ONE_BYTE)::value>
            <<<dim3(sh.blocks), dim3(sh.block), scan_dyn_lds(sh), st>>>(pr, la, sh.tpb, bound);
    });
}

}  // namespace ss
