// scan_inst_nocase.hip - the case-folding scans (nocase_kernels.hpp): one scan_all_nocase_kernel and one lines_scan_nocase_kernel
// per (Q, MODE, one-byte) combination their models have - 4 Q x MODE 0, 4 Q x MODE 2, one-byte: 9 each.  Compiled into
// libsliceslice_hip_nocase.so only (ss_nocase.hip is the host side).
#include "nocase_kernels.hpp"
#include "nocase_launch.hpp"

namespace ss {

namespace {

template <int Q, int MODE, bool ONE_BYTE>
void launch_all_nocase_one(const Problem &pr, const Shape &sh, hipStream_t st, const AllArgs &aa)
{
    const uint32_t dyn_lds = sh.lds_pad + (sh.block / kWave) * kNeedleLds;   // one needle slice per wave
    scan_all_nocase_kernel<Q, MODE, ONE_BYTE><<<dim3(sh.blocks), dim3(sh.block), dyn_lds, st>>>(pr, aa, sh.tpb);
}

template <int Q, int MODE, bool ONE_BYTE>
void launch_lines_nocase_one(const Problem &pr, const Shape &sh, hipStream_t st, const LineArgs &la)
{
    const uint32_t dyn_lds = sh.lds_pad + (sh.block / kWave) * kNeedleLds;
    lines_scan_nocase_kernel<Q, MODE, ONE_BYTE><<<dim3(sh.blocks), dim3(sh.block), dyn_lds, st>>>(pr, la, sh.tpb);
}

}  // namespace

#define SS_CASE(QQ, MM)                                                                            \
    case (QQ) * 4 + (MM):                                                                          \
        return SS_ONE<QQ, MM, false>(pr, sh, st, args), true;
#define SS_CASES                                                                                   \
    if (one_byte) return SS_ONE<0, 0, true>(pr, sh, st, args), true;                               \
    if (mode == 3) mode = 2;                  /* a pair-alone searcher: the MODE 2 kernel, as the models do */ \
    switch (q * 4 + mode) {                                                                        \
        SS_CASE(0, 0) SS_CASE(0, 2) SS_CASE(1, 0) SS_CASE(1, 2)                                    \
        SS_CASE(2, 0) SS_CASE(2, 2) SS_CASE(3, 0) SS_CASE(3, 2)                                    \
    }                                                                                              \
    return false;

bool launch_scan_all_nocase(const Problem &pr, int q, int mode, bool one_byte, const Shape &sh, hipStream_t st, const AllArgs &args)
{
#define SS_ONE launch_all_nocase_one
    SS_CASES
#undef SS_ONE
}

bool launch_scan_lines_nocase(const Problem &pr, int q, int mode, bool one_byte, const Shape &sh, hipStream_t st, const LineArgs &args)
{
#define SS_ONE launch_lines_nocase_one
    SS_CASES
#undef SS_ONE
}
#undef SS_CASES
#undef SS_CASE

}  // namespace ss
