// scan_inst_inverted.hip - the case-sensitive inverted emit kernels (inverted_kernels.hpp): one lines_emit_inverted_kernel per
// (Q, MODE, one-byte) combination of scan_choice.hpp, without and with the neighbour test - 9 x 2 = 18 - plus the two small kernels
// (inverted_small_kernels.hpp).  Compiled into libsliceslice_hip_inverted.so only (ss_inverted.hip is the host side); the folding
// ones are scan_inst_inverted_nocase.hip's, so that the two halves compile side by side.
#include "inverted_small_kernels.hpp"
#include "scan_choice.hpp"

namespace ss {

bool launch_emit_lines_inverted(const Problem &pr, int q, int mode, bool one_byte, const Shape &sh, hipStream_t st, const LineArgs &la, uint32_t bound)
{
    return choose_scan_kernel(q, mode, one_byte, [&](auto Q, auto MODE, auto ONE_BYTE) {
        if (bound != 0)
            lines_emit_inverted_kernel<decltype(Q)::value, decltype(MODE)::value, decltype(ONE_BYTE)::value, false, true>
                <<<dim3(sh.blocks), dim3(sh.block), scan_dyn_lds(sh), st>>>(pr, la, sh.tpb, bound);
        else
            lines_emit_inverted_kernel<decltype(Q)::value, decltype(MODE)::value, decltype(ONE_BYTE)::value, false, false>
                <<<dim3(sh.blocks), dim3(sh.block), scan_dyn_lds(sh), st>>>(pr, la, sh.tpb, bound);
    });
}

hipError_t launch_lines_plain_inverted(const PlainArgs &pa, hipStream_t st)
{
    const uint64_t parts = pa.end > pa.begin ? (pa.end - pa.begin + pa.part_bytes - 1) / pa.part_bytes : 1;
    lines_plain_inverted_kernel<<<(unsigned)parts, kBlock, 0, st>>>(pa);
    return hipGetLastError();
}

hipError_t launch_lines_total_inverted(const CombineArgs &ca, hipStream_t st)
{
    lines_total_inverted_kernel<<<1, 1, 0, st>>>(ca);
    return hipGetLastError();
}

}  // namespace ss
