// lines_launch.hpp - host-side entry points and argument blocks of the matching-lines kernels (lines_kernels.hpp; defined in
// scan_inst_lines.hip, used by ss_lines.hip).
#pragma once
#include "scan_launch.hpp"

namespace ss {

constexpr uint32_t kLinesSum = 0, kLinesEmit = 1;
constexpr int kLineChunk = 256;          // parts per workgroup of lines_chunk_kernel

struct LineArgs {
    LineSum *sum;               // kLinesSum: written, sum[part0 + workgroup]
    const LinePre *pre;         // kLinesEmit: read, pre[part0 + workgroup]
    uint64_t *begin, *end, *number;     // kLinesEmit: the caller's arrays (each may be null), ranks below capacity only
    uint64_t capacity;
    uint64_t dlo, dhi;          // stream positions of the view's first byte and of its end
    int64_t hshift;             // hay index = stream position + hshift
    uint64_t part0;
    uint32_t delim;
    uint32_t mode;
};

// lines_plain_kernel: bytes [begin, end) of the haystack, parts of part_bytes, one workgroup each
struct PlainArgs {
    const uint8_t *hay;
    uint64_t begin, end, part_bytes;
    LineSum *sum;
    const LinePre *pre;
    uint64_t *out_begin, *out_end, *out_number;
    uint64_t capacity;
    uint64_t part0;
    uint32_t delim;
    uint32_t mode;
};

// lines_combine_kernel: the n parts' summaries -> the state in front of each, the total, an unterminated last line's record
struct CombineArgs {
    const LineSum *sum;
    uint64_t n;
    LinePre *pre;
    uint64_t *total, *total2;
    uint64_t len;
    uint64_t *out_begin, *out_end, *out_number;
    uint64_t capacity;
};

// The matching-lines scan of one Problem (the kernel choice of launch_scan_all: scan_choice.hpp).  Returns false when no kernel fits.
// (`bound`: as for launch_scan_all - 0, ignored)
bool launch_scan_lines(const Problem &pr, int q, int mode, bool one_byte, const Shape &sh, hipStream_t st, const LineArgs &la, uint32_t bound);
// (the host side takes the scan as a value of this type: ss_lines.hip, lines_host.hpp)
typedef bool (*ScanLinesFn)(const Problem &pr, int q, int mode, bool one_byte, const Shape &sh, hipStream_t st, const LineArgs &la, uint32_t bound);
// ceil((end - begin) / part_bytes) workgroups (at least one: an empty range leaves an empty summary)
hipError_t launch_lines_plain(const PlainArgs &pa, bool every, hipStream_t st);
// The summaries of `n` parts in chunks of kLineChunk: csum[chunk] = the chunk's summary (spread == false), or - behind the combine
// over the chunks - pre[k] = the state in front of every part from cpre[chunk] (spread == true).
hipError_t launch_lines_chunks(const LineSum *sum, uint64_t n, LineSum *csum, const LinePre *cpre, LinePre *pre, bool spread, hipStream_t st);
hipError_t launch_lines_combine(const CombineArgs &ca, hipStream_t st);

}  // namespace ss
