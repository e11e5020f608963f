// lines_kernels.hpp - the kernels of the matching-lines calls (include/sliceslice_hip_lines.h; libsliceslice_hip_lines.so only:
// scan_inst_lines.hip instantiates them, ss_lines.hip is the host side).
//
//   lines_scan_kernel     scan_all_kernel's scan (scan_tiles<..., ALL, LINES>: the find kernels' filter and verification, no early
//                         exit) plus the delimiter filter and the segmented combine of lines_tiles.hpp.  kLinesSum: ONE pass over the
//                         haystack that leaves one LineSum per workgroup.  kLinesEmit: the same grid again; only the workgroups that
//                         close one of the first `capacity` matching lines re-read their tiles and write the records at their rank.
//   lines_plain_kernel    the same two modes for bytes that hold no match by construction - the few in front of and behind the filter
//                         stream (the stream starts at the first filter byte and ends with the last candidate's tile) - and for the
//                         empty needle, which matches every line (EVERY).
//   lines_chunk_kernel    the parts' summaries in chunks of kLineChunk, one workgroup per chunk: the chunk's summary, and - behind the
//                         combine, for the emit launches - the state in front of every part (LinePre).
//   lines_combine_kernel  ONE workgroup over the chunks' summaries, in the style of prefix_kernel.hpp: the state in front of every
//                         chunk, the total, and the record of an unterminated last line.  It walks parts / kLineChunk entries, so the
//                         only launch whose duration follows the haystack is the scan.
// Scratch is one LineSum and one LinePre per workgroup and per chunk; nothing is kept per match, per line or per delimiter, and there is no global
// atomic anywhere.
#pragma once
#include "lines_launch.hpp"
#include "lines_scan_body.hpp"

namespace ss {


// Contiguous tiles per workgroup (1 <= tiles_per_block <= kLineTilesPerBlock), so that workgroup order is address order.
// (lines_scan_body.hpp holds the text, shared with the case-folding twin of nocase_kernels.hpp)
SS_LINES_SCAN_KERNEL(lines_scan_kernel, false)

// Bytes [begin, end) of the haystack in parts of part_bytes, one workgroup each (thread t: a contiguous run of the part).  No match
// inside (EVERY = false: only a pending match in front of a part closes a line, at the part's first delimiter) or every line
// matches (EVERY = true: the empty needle).

template <bool EVERY>
__global__ void __launch_bounds__(kBlock) lines_plain_kernel(PlainArgs pa)
{
    __shared__ uint64_t s_cnt[kBlock], s_lastd[kBlock];
    const uint64_t p0 = pa.begin + (uint64_t)blockIdx.x * pa.part_bytes;
    const uint64_t p1 = p0 + pa.part_bytes < pa.end ? p0 + pa.part_bytes : pa.end;
    const uint64_t per = (pa.part_bytes + kBlock - 1) / kBlock;
    const uint64_t b0 = p0 + (uint64_t)threadIdx.x * per, b = b0 < p1 ? b0 : p1, e = b + per < p1 ? b + per : p1;
    const uint8_t dl = (uint8_t)pa.delim;
    LinePre at = {0, 0, 0, 0, 0};
    if (pa.mode == kLinesEmit) {
        at = pa.pre[pa.part0 + blockIdx.x];
        if (at.closes == 0 || at.rank >= pa.capacity) return;           // (workgroup-uniform)
    }
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
    if (pa.mode == kLinesSum) {
        if (threadIdx.x == 0) {
            LineSum sum = {0, 0, 0, 0, 0};
            for (int t = 0; t < kBlock; ++t) {
                sum.ndelim += s_cnt[t];
                if (s_lastd[t]) sum.last = s_lastd[t];
            }
            if (sum.ndelim) sum.flags = kLineHas;
            if (EVERY && p1 > p0) {
                sum.flags |= kLineHead;
                if (sum.last < p1) sum.flags |= kLineTail;              // bytes behind the last delimiter: a line is open
                if (sum.ndelim) sum.closed = sum.ndelim - 1;
            }
            pa.sum[pa.part0 + blockIdx.x] = sum;
        }
        return;
    }
    // emit: delimiters and the open line in front of this thread's run
    uint64_t before = 0, open = at.last;
    for (unsigned t = 0; t < threadIdx.x; ++t) {
        before += s_cnt[t];
        if (s_lastd[t]) open = s_lastd[t];
    }
    for (uint64_t i = b; i < e; ++i) {
        if (pa.hay[i] != dl) continue;
        const bool closes = EVERY || (before == 0 && at.carry != 0);
        const uint64_t r = at.rank + (EVERY ? before : 0);
        if (closes && r < pa.capacity) {
            if (pa.out_begin) pa.out_begin[r] = open;
            if (pa.out_end) pa.out_end[r] = i;
            if (pa.out_number) pa.out_number[r] = at.ndelim + before + 1;
        }
        open = i + 1;
        ++before;
    }
}

// The parts' summaries in chunks of kLineChunk, one workgroup per chunk (thread t: part chunk * kLineChunk + t; an inclusive scan of
// the chunk in LDS).  SPREAD = false: csum[chunk] = the chunk's summary - what lines_combine_kernel then scans, so that its one
// workgroup walks parts / kLineChunk entries.  SPREAD = true (find only, behind the combine): pre[k] = the state in front of part k,
// from the state in front of its chunk (cpre) and the parts of the chunk before it.
template <bool SPREAD>
__global__ void __launch_bounds__(kLineChunk) lines_chunk_kernel(const LineSum *sum, uint64_t n, LineSum *csum, const LinePre *cpre, LinePre *pre)
{
    __shared__ LineSum s_part[kLineChunk];
    const uint64_t k = (uint64_t)blockIdx.x * kLineChunk + threadIdx.x;
    LineSum mine = {0, 0, 0, 0, 0};
    if (k < n) mine = sum[k];
    s_part[threadIdx.x] = mine;
    __syncthreads();
    for (int d = 1; d < kLineChunk; d <<= 1) {                  // Hillis-Steele inclusive scan
        LineSum v = {0, 0, 0, 0, 0};
        if (threadIdx.x >= (unsigned)d) v = s_part[threadIdx.x - d];
        __syncthreads();
        s_part[threadIdx.x] = line_combine(v, s_part[threadIdx.x]);
        __syncthreads();
    }
    if constexpr (!SPREAD) {
        if (threadIdx.x == kLineChunk - 1) csum[blockIdx.x] = s_part[threadIdx.x];
    } else {
        if (k >= n) return;
        LinePre at = cpre[blockIdx.x];
        if (threadIdx.x > 0) (void)line_advance(at, s_part[threadIdx.x - 1]);
        LinePre p = at;
        const uint64_t c = line_advance(at, mine);
        p.closes = c > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)c;
        pre[k] = p;
    }
}

// pre[k] = the state in front of part k, *total (and *total2 when not null) = the number of matching lines; the record of an
// unterminated last line (it has no delimiter to belong to) is written here.  One workgroup, as prefix_kernel: thread t combines a
// contiguous run of the summaries, the runs' summaries are scanned in LDS, and every thread walks its run again.
constexpr int kCombineThreads = 1024;

__global__ void __launch_bounds__(kCombineThreads) lines_combine_kernel(CombineArgs ca)
{
    __shared__ LineSum s_run[kCombineThreads];
    const uint64_t per = (ca.n + kCombineThreads - 1) / kCombineThreads;
    const uint64_t b0 = (uint64_t)threadIdx.x * per, b = b0 < ca.n ? b0 : ca.n, e = b + per < ca.n ? b + per : ca.n;
    LineSum run = {0, 0, 0, 0, 0};
    for (uint64_t k = b; k < e; ++k) run = line_combine(run, ca.sum[k]);
    s_run[threadIdx.x] = run;
    __syncthreads();
    for (int k = 1; k < kCombineThreads; k <<= 1) {             // Hillis-Steele inclusive scan of the runs
        LineSum v = {0, 0, 0, 0, 0};
        if (threadIdx.x >= (unsigned)k) v = s_run[threadIdx.x - k];
        __syncthreads();
        s_run[threadIdx.x] = line_combine(v, s_run[threadIdx.x]);
        __syncthreads();
    }
    LinePre at = {0, 0, 0, 0, 0};
    if (threadIdx.x > 0) (void)line_advance(at, s_run[threadIdx.x - 1]);
    for (uint64_t k = b; k < e; ++k) {
        LinePre p = at;
        const uint64_t c = line_advance(at, ca.sum[k]);
        p.closes = c > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)c;
        ca.pre[k] = p;
    }
    if (threadIdx.x == kCombineThreads - 1) {
        LinePre fin = {0, 0, 0, 0, 0};
        (void)line_advance(fin, s_run[threadIdx.x]);
        uint64_t total = fin.rank;
        if (fin.carry && fin.last < ca.len) {                   // the last line has no delimiter and holds a match
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
}

}  // namespace ss
