// scan_inst_lines.hip - the matching-lines kernels (lines_kernels.hpp): one lines_scan_kernel per (Q, MODE, one-byte) combination
// that find_all() has - 4 Q x MODE 0, 4 Q x MODE 2, one-byte: 9, chosen by scan_choice.hpp - plus the plain, chunk and combine kernels.  Compiled into
// libsliceslice_hip_lines.so only (ss_lines.hip is the host side).
#include "lines_kernels.hpp"
#include "scan_choice.hpp"

namespace ss {

bool launch_scan_lines(const Problem &pr, int q, int mode, bool one_byte, const Shape &sh, hipStream_t st, const LineArgs &la, uint32_t)
{
    return choose_scan_kernel(q, mode, one_byte, [&](auto Q, auto MODE, auto ONE_BYTE) {
        lines_scan_kernel<decltype(Q)::value, decltype(MODE)::value, decltype(ONE_BYTE)::value>
            <<<dim3(sh.blocks), dim3(sh.block), scan_dyn_lds(sh), st>>>(pr, la, sh.tpb);
    });
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
