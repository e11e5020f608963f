// scan_inst_nocase.hip - the case-folding scans (nocase_kernels.hpp): one scan_all_nocase_kernel and one lines_scan_nocase_kernel
// per (Q, MODE, one-byte) combination their models have - 4 Q x MODE 0, 4 Q x MODE 2, one-byte: 9 each, chosen by scan_choice.hpp.  Compiled into
// libsliceslice_hip_nocase.so only (ss_nocase.hip is the host side).
#include "nocase_kernels.hpp"
#include "nocase_launch.hpp"
#include "scan_choice.hpp"

namespace ss {

bool launch_scan_all_nocase(const Problem &pr, int q, int mode, bool one_byte, const Shape &sh, hipStream_t st, const AllArgs &aa, uint32_t)
{
    return choose_scan_kernel(q, mode, one_byte, [&](auto Q, auto MODE, auto ONE_BYTE) {
        scan_all_nocase_kernel<decltype(Q)::value, decltype(MODE)::value, decltype(ONE_BYTE)::value>
            <<<dim3(sh.blocks), dim3(sh.block), scan_dyn_lds(sh), st>>>(pr, aa, sh.tpb);
    });
}

bool launch_scan_lines_nocase(const Problem &pr, int q, int mode, bool one_byte, const Shape &sh, hipStream_t st, const LineArgs &la, uint32_t)
{
    return choose_scan_kernel(q, mode, one_byte, [&](auto Q, auto MODE, auto ONE_BYTE) {
        lines_scan_nocase_kernel<decltype(Q)::value, decltype(MODE)::value, decltype(ONE_BYTE)::value>
            <<<dim3(sh.blocks), dim3(sh.block), scan_dyn_lds(sh), st>>>(pr, la, sh.tpb);
    });
}

}  // namespace ss
