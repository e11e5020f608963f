// nocase_kernels.hpp - the case-folding twins of the all-matches and matching-lines scans (include/sliceslice_hip_nocase.h;
// libsliceslice_hip_nocase.so only: scan_inst_nocase.hip instantiates them, ss_nocase.hip is the host side).
//
// Both are their models' text (scan_all_body, SS_LINES_SCAN_KERNEL) with scan_tiles<..., FOLD = true>: every loaded register
// goes through fold_ascii4 once, right behind the load - 'A'..'Z' become 'a'..'z', every other byte value stays - and the places
// that read haystack bytes from memory (verify_candidate, same_bytes, the one-byte test, the far filter byte) fold them there.
// The searcher's needle holds no upper-case byte (the host checks), so the filters, the second level and the compares are the
// case-sensitive ones on folded bytes.  The lines kernel takes its delimiter masks from the RAW registers: the delimiter is never
// folded.  The small kernels around the scans (prefix sum, plain parts, chunks, combine) never compare needle bytes and are the
// models' own.
#pragma once
#include "lines_scan_body.hpp"

namespace ss {

template <int Q, int MODE, bool ONE_BYTE>
__global__ void __launch_bounds__(kMaxBlock) scan_all_nocase_kernel(const Problem pr, AllArgs aa, uint64_t tiles_per_block)
{
    scan_all_body<Q, MODE, ONE_BYTE, true>(pr, aa, tiles_per_block);
}

SS_LINES_SCAN_KERNEL(lines_scan_nocase_kernel, true)

}  // namespace ss
