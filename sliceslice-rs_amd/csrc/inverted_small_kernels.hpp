// inverted_small_kernels.hpp - the two small kernels of the inverted matching-lines calls (inverted_kernels.hpp has the overview).
// Not templates, so exactly one translation unit includes this file: scan_inst_inverted.hip.
#pragma once
#include "inverted_kernels.hpp"

namespace ss {

// lines_plain_kernel<false>'s emit half with the selection complemented: bytes [begin, end) of the haystack in parts of
// part_bytes, one workgroup each (thread t: a contiguous run of the part), no match inside.
__global__ void __launch_bounds__(kBlock) lines_plain_inverted_kernel(PlainArgs pa)
{
    __shared__ uint64_t s_cnt[kBlock], s_lastd[kBlock];
    const uint64_t p0 = pa.begin + (uint64_t)blockIdx.x * pa.part_bytes;
    const uint64_t p1 = p0 + pa.part_bytes < pa.end ? p0 + pa.part_bytes : pa.end;
    const uint64_t per = (pa.part_bytes + kBlock - 1) / kBlock;
    const uint64_t b0 = p0 + (uint64_t)threadIdx.x * per, b = b0 < p1 ? b0 : p1, e = b + per < p1 ? b + per : p1;
    const uint8_t dl = (uint8_t)pa.delim;
    const LinePre at = pa.pre[pa.part0 + blockIdx.x];
    const uint64_t rank0 = at.ndelim - at.rank;                         // lines without a match closed in front of the part
    if (rank0 >= pa.capacity) return;                                   // (workgroup-uniform)
    uint64_t cnt = 0, lastd = 0;
    for (uint64_t i = b; i < e; ++i) {
        if (pa.hay[i] == dl) {
            ++cnt;
            lastd = i + 1;
        }
    }
    s_cnt[threadIdx.x] = cnt;
    s_lastd[threadIdx.x] = lastd;
    __syncthreads();
    // delimiters and the open line in front of this thread's run
    uint64_t before = 0, open = at.last;
    for (unsigned t = 0; t < threadIdx.x; ++t) {
        before += s_cnt[t];
        if (s_lastd[t]) open = s_lastd[t];
    }
    const uint64_t pending = at.carry != 0 ? 1u : 0u;                   // the part's first delimiter closes a line with a match
    for (uint64_t i = b; i < e; ++i) {
        if (pa.hay[i] != dl) continue;
        if (before >= pending) {
            const uint64_t r = rank0 + before - pending;
            if (r < pa.capacity) {
                if (pa.out_begin) pa.out_begin[r] = open;
                if (pa.out_end) pa.out_end[r] = i;
                if (pa.out_number) pa.out_number[r] = at.ndelim + before + 1;
            }
        }
        open = i + 1;
        ++before;
    }
}

// Behind lines_combine_kernel over the same ca.n >= 1 summaries: ca.pre[k] is the state in front of summary k as that kernel
// left it.  *total (and *total2 when not null) = the number of lines without a match; an unterminated last line is one of them
// when no match is pending at the end of the view, and its record - it has no delimiter to belong to - is written here.
__global__ void lines_total_inverted_kernel(CombineArgs ca)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    LinePre fin = ca.pre[ca.n - 1];
    (void)line_advance(fin, ca.sum[ca.n - 1]);
    uint64_t total = fin.ndelim - fin.rank;
    if (fin.last < ca.len && fin.carry == 0) {
        if (total < ca.capacity) {
            if (ca.out_begin) ca.out_begin[total] = fin.last;
            if (ca.out_end) ca.out_end[total] = ca.len;
            if (ca.out_number) ca.out_number[total] = fin.ndelim + 1;
        }
        ++total;
    }
    *ca.total = total;
    if (ca.total2) *ca.total2 = total;
}

}  // namespace ss
