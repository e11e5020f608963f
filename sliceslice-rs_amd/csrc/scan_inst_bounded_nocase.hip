// scan_inst_bounded_nocase.hip - the case-folding whole-word / whole-line scans (bounded_kernels.hpp with scan_tiles' FOLD switch
// on, as nocase_kernels.hpp has it): one scan_all_bounded_kernel<..., FOLD = true> and one lines_scan_bounded_nocase_kernel per
// (Q, MODE, one-byte) combination - 9 each, chosen by scan_choice.hpp.  Compiled into libsliceslice_hip_bounded.so only.
#include "bounded_kernels.hpp"
#include "bounded_launch.hpp"
#include "scan_choice.hpp"

namespace ss {

bool launch_scan_all_bounded_nocase(const Problem &pr, int q, int mode, bool one_byte, const Shape &sh, hipStream_t st, const AllArgs &aa, uint32_t bound)
{
    return choose_scan_kernel(q, mode, one_byte, [&](auto Q, auto MODE, auto ONE_BYTE) {
        scan_all_bounded_kernel<decltype(Q)::value, decltype(MODE)::value, decltype(ONE_BYTE)::value, true>
            <<<dim3(sh.blocks), dim3(sh.block), scan_dyn_lds(sh), st>>>(pr, aa, sh.tpb, bound);
    });
}

bool launch_scan_lines_bounded_nocase(const Problem &pr, int q, int mode, bool one_byte, const Shape &sh, hipStream_t st, const LineArgs &la, uint32_t bound)
{
    return choose_scan_kernel(q, mode, one_byte, [&](auto Q, auto MODE, auto ONE_BYTE) {
        lines_scan_bounded_nocase_kernel<decltype(Q)::value, decltype(MODE)::value, decltype(ONE_BYTE)::value>
            <<<dim3(sh.blocks), dim3(sh.block), scan_dyn_lds(sh), st>>>(pr, la, sh.tpb, bound);
    });
}

}  // namespace ss
