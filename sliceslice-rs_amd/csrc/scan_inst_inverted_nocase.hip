// scan_inst_inverted_nocase.hip - the case-folding inverted emit kernels (inverted_kernels.hpp with scan_tiles' FOLD switch on):
// one lines_emit_inverted_kernel<..., FOLD = true> per (Q, MODE, one-byte) combination of scan_choice.hpp, without and with the
// neighbour test - 9 x 2 = 18.  Compiled into libsliceslice_hip_inverted.so only.
#include "inverted_kernels.hpp"
#include "scan_choice.hpp"

namespace ss {

bool launch_emit_lines_inverted_nocase(const Problem &pr, int q, int mode, bool one_byte, const Shape &sh, hipStream_t st, const LineArgs &la, uint32_t bound)
{
    return choose_scan_kernel(q, mode, one_byte, [&](auto Q, auto MODE, auto ONE_BYTE) {
        if (bound != 0)
            lines_emit_inverted_kernel<decltype(Q)::value, decltype(MODE)::value, decltype(ONE_BYTE)::value, true, true>
                <<<dim3(sh.blocks), dim3(sh.block), scan_dyn_lds(sh), st>>>(pr, la, sh.tpb, bound);
        else
            lines_emit_inverted_kernel<decltype(Q)::value, decltype(MODE)::value, decltype(ONE_BYTE)::value, true, false>
                <<<dim3(sh.blocks), dim3(sh.block), scan_dyn_lds(sh), st>>>(pr, la, sh.tpb, bound);
    });
}

}  // namespace ss
