// scan_inst_lines.hip - the matching-lines kernels (lines_kernels.hpp): one lines_scan_kernel per (Q, MODE, one-byte) combination
// that find_all() has - 4 Q x MODE 0, 4 Q x MODE 2, one-byte: 9 - plus the plain, chunk and combine kernels.  Compiled into
// libsliceslice_hip_lines.so only (ss_lines.hip is the host side).
#include "lines_kernels.hpp"

namespace ss {

namespace {

template <int Q, int MODE, bool ONE_BYTE>
void launch_lines_one(const Problem &pr, const Shape &sh, hipStream_t st, const LineArgs &la)
{
    const uint32_t dyn_lds = sh.lds_pad + (sh.block / kWave) * kNeedleLds;   // one needle slice per wave
    lines_scan_kernel<Q, MODE, ONE_BYTE><<<dim3(sh.blocks), dim3(sh.block), dyn_lds, st>>>(pr, la, sh.tpb);
}

}  // namespace

bool launch_scan_lines(const Problem &pr, int q, int mode, bool one_byte, const Shape &sh, hipStream_t st, const LineArgs &la)
{
    if (one_byte) return launch_lines_one<0, 0, true>(pr, sh, st, la), true;
    if (mode == 3) mode = 2;                  // a pair-alone searcher: the MODE 2 kernel with its third byte, as find_all() does
#define SS_CASE(QQ, MM)                                                                            \
    case (QQ) * 4 + (MM):                                                                          \
        return launch_lines_one<QQ, MM, false>(pr, sh, st, la), true;
    switch (q * 4 + mode) {
        SS_CASE(0, 0) SS_CASE(0, 2) SS_CASE(1, 0) SS_CASE(1, 2)
        SS_CASE(2, 0) SS_CASE(2, 2) SS_CASE(3, 0) SS_CASE(3, 2)
    }
#undef SS_CASE
    return false;
}

hipError_t launch_lines_plain(const PlainArgs &pa, bool every, hipStream_t st)
{
    uint64_t parts = pa.end > pa.begin ? (pa.end - pa.begin + pa.part_bytes - 1) / pa.part_bytes : 1;
    if (every) lines_plain_kernel<true><<<(unsigned)parts, kBlock, 0, st>>>(pa);
    else lines_plain_kernel<false><<<(unsigned)parts, kBlock, 0, st>>>(pa);
    return hipGetLastError();
}

hipError_t launch_lines_chunks(const LineSum *sum, uint64_t n, LineSum *csum, const LinePre *cpre, LinePre *pre, bool spread, hipStream_t st)
{
    const unsigned chunks = (unsigned)((n + kLineChunk - 1) / kLineChunk);
    if (spread) lines_chunk_kernel<true><<<chunks, kLineChunk, 0, st>>>(sum, n, csum, cpre, pre);
    else lines_chunk_kernel<false><<<chunks, kLineChunk, 0, st>>>(sum, n, csum, cpre, pre);
    return hipGetLastError();
}

hipError_t launch_lines_combine(const CombineArgs &ca, hipStream_t st)
{
    lines_combine_kernel<<<1, kCombineThreads, 0, st>>>(ca);
    return hipGetLastError();
}

}  // namespace ss
