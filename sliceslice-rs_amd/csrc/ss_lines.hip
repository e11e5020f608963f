// ss_lines.hip - the lines that contain a needle (include/sliceslice_hip_lines.h): ss_count_lines_device / _async,
// ss_find_lines_device.  NOT in the other libraries: libsliceslice_hip_lines.so holds the matches library's objects plus this file
// and scan_inst_lines.hip.
//
// The view is cut into PARTS in address order: the bytes in front of the filter stream (the stream starts at the first filter
// byte, which need not be the needle's first), one part per workgroup of the scan, and the bytes behind the last candidate's tile.
//   count   the two edge parts (lines_plain_kernel; a few bytes, no match inside by construction), ONE scan launch that leaves a
//           summary per workgroup (lines_scan_kernel), and the combine over the summaries: one workgroup per 256 of them
//           (lines_chunk_kernel), then one workgroup over those (lines_combine_kernel).
//   find    the same, then the emit launches over the same grids: only the parts that close one of the first `capacity` matching
//           lines read their bytes again and write the records at their rank.  A line longer than a tile, a workgroup's run or
//           several of them is carried by the summaries alone.
// The empty needle matches every line: the plain kernel in its EVERY form over the whole view, same combine.
// The inverse of a call - the lines WITHOUT a match, ss_inverted.hip - is the same sum pass and, in place of the emit launches and
// behind the combine, the three launches its LinesInverted names (lines_host.hpp); this file holds none of those kernels.
// The launch shape is ss_matches.hip's (plan_static: the static one of an untuned search); the census is neither started nor read.
#include "ss_internal.hpp"

#include "../../include/sliceslice_hip_lines.h"
#include "lines_host.hpp"
#include "matches_host.hpp"
#include "matches_scratch.hpp"

#include <algorithm>

namespace ssh {
namespace {

constexpr uint64_t kPlainPart = 64 * 1024;          // bytes per workgroup of the empty needle's pass

// ss_matches.hip's plan with the tiles per workgroup capped and the edges of the filter stream
struct LinesLaunch : StaticPlan {
    uint64_t head_end = 0, tail_begin = 0;          // hay [0, head_end) and [tail_begin, len) are not part of the filter stream
    uint64_t dlo = 0, dhi = 0;
    int64_t hshift = 0;
};

int plan_lines(const ss_searcher *s, PerDevice *pd, const void *d_hay, size_t len, LinesLaunch *out)
{
    if (int rc = plan_static(s, pd, d_hay, len, out)) return rc;
    if (out->shape.tpb > (uint64_t)ss::kLineTilesPerBlock) {
        // a workgroup keeps its waves' summaries of at most kLineTilesPerBlock tiles in LDS: whatever launch_grid's tuning prefers,
        // the answer must not depend on it
        const uint64_t blocks = (out->ntiles + ss::kLineTilesPerBlock - 1) / ss::kLineTilesPerBlock;
        if (blocks > 0x7fffffffull)
            return fail(SS_ERR_ARGUMENT, "a haystack of %zu bytes needs %llu workgroups of %d tiles; a grid holds 2^31 - 1", len,
                        (unsigned long long)blocks, ss::kLineTilesPerBlock);
        out->shape.tpb = ss::kLineTilesPerBlock;
        out->shape.blocks = (unsigned)blocks;
    }
    // stream position a holds hay[a + fa - mis]; every wave of every tile loads its chunks below nchunks_all
    const uint64_t fa = out->ps.fa, mis = out->pr.mis;
    const uint64_t covered = std::min(out->ntiles * kPiecesPerTile * 1024, out->pr.nchunks_all * 16);
    out->hshift = (int64_t)fa - (int64_t)mis;
    out->head_end = fa > mis ? fa - mis : 0;
    out->tail_begin = std::min<uint64_t>(len, (uint64_t)((int64_t)covered + out->hshift));
    out->dlo = mis > fa ? mis - fa : 0;
    out->dhi = (uint64_t)((int64_t)len - out->hshift);
    return SS_OK;
}

// [total, 32 bytes][LineSum x parts][LinePre x parts][LineSum x chunks][LinePre x chunks]
struct LinesScratch {
    uint64_t parts = 0, chunks = 0;
    uint64_t *total = nullptr;
    ss::LineSum *sum = nullptr, *csum = nullptr;
    ss::LinePre *pre = nullptr, *cpre = nullptr;
};

int take_lines_scratch(int dev, uint64_t parts, hipStream_t st, ScratchLease *lease, LinesScratch *out)
{
    const uint64_t chunks = (parts + ss::kLineChunk - 1) / ss::kLineChunk;
    if (int rc = take_scratch(dev, 32 + (parts + chunks) * (sizeof(ss::LineSum) + sizeof(ss::LinePre)), &lease->sc, st)) return rc;
    out->parts = parts;
    out->chunks = chunks;
    out->total = reinterpret_cast<uint64_t *>(lease->sc.d);
    out->sum = reinterpret_cast<ss::LineSum *>(lease->sc.d + 32);
    out->pre = reinterpret_cast<ss::LinePre *>(out->sum + parts);
    out->csum = reinterpret_cast<ss::LineSum *>(out->pre + parts);
    out->cpre = reinterpret_cast<ss::LinePre *>(out->csum + chunks);
    return SS_OK;
}

struct LinesOut {
    uint64_t *begin = nullptr, *end = nullptr, *number = nullptr;
    uint64_t capacity = 0;
    uint64_t *d_total2 = nullptr;       // the async count's destination
};

// The parts' summaries -> the total (and the record of an unterminated last line), and - for the emit launches - the state in front
// of every part: chunk summaries (many workgroups), ONE workgroup over the chunks, and the states spread back over the chunks.
// inv: the model's combine leaves its states and writes no record (capacity 0) and no second total; the total, the second one and the
// last line's record are the inverted ones of inv->total behind it.
int combine_parts(const LinesScratch &sc, size_t len, const LinesOut &o, bool emit, hipStream_t st, const LinesInverted *inv)
{
    HIP_TRY(ss::launch_lines_chunks(sc.sum, sc.parts, sc.csum, sc.cpre, sc.pre, false, st));
    ss::CombineArgs ca = {sc.csum, sc.chunks, sc.cpre, sc.total, inv ? nullptr : o.d_total2, len, o.begin, o.end, o.number,
                          emit && !inv ? o.capacity : 0};
    HIP_TRY(ss::launch_lines_combine(ca, st));
    if (inv) {
        ca.total2 = o.d_total2;
        ca.capacity = emit ? o.capacity : 0;
        HIP_TRY(inv->total(ca, st));
    }
    if (emit) HIP_TRY(ss::launch_lines_chunks(sc.sum, sc.parts, sc.csum, sc.cpre, sc.pre, true, st));
    return SS_OK;
}

// Enqueues everything; *d_total = the scratch word that takes the total.  Preconditions: len >= 1, and either every line is
// selected (`every`: the empty needle - or, for an inverted call, a needle that no line can hold) or the needle holds no delimiter and
// n <= len.  inv: the inverse of the call (lines_host.hpp), never together with `every`.
int enqueue_lines(ss::ScanLinesFn scan, const ss_searcher *s, PerDevice *pd, const void *d_hay, size_t len, int delimiter, hipStream_t st, const LinesOut &o,
                  ScratchLease *lease, uint64_t **d_total, uint32_t bound, bool every, const LinesInverted *inv)
{
    const uint8_t *hay = static_cast<const uint8_t *>(d_hay);
    const bool emit = o.capacity != 0 && (o.begin || o.end || o.number);
    if (every) {
        const uint64_t parts = (len + kPlainPart - 1) / kPlainPart;
        if (parts > 0x7fffffffull) return fail(SS_ERR_ARGUMENT, "haystack of %zu bytes is too long for the empty needle's pass", len);
        LinesScratch sc;
        if (int rc = take_lines_scratch(pd->dev, parts, st, lease, &sc)) return rc;
        *d_total = sc.total;
        ss::LineSum *sum = sc.sum;
        ss::LinePre *pre = sc.pre;
        ss::PlainArgs pa = {hay, 0, len, kPlainPart, sum, pre, o.begin, o.end, o.number, o.capacity, 0, (uint32_t)delimiter, ss::kLinesSum};
        HIP_TRY(ss::launch_lines_plain(pa, true, st));
        if (int rc = combine_parts(sc, len, o, emit, st, nullptr)) return rc;
        if (emit) {
            pa.mode = ss::kLinesEmit;
            HIP_TRY(ss::launch_lines_plain(pa, true, st));
        }
        return SS_OK;
    }
    LinesLaunch ll;
    if (int rc = plan_lines(s, pd, d_hay, len, &ll)) return rc;
    const uint64_t blocks = ll.shape.blocks, parts = blocks + 2;
    LinesScratch sc;
    if (int rc = take_lines_scratch(pd->dev, parts, st, lease, &sc)) return rc;
    *d_total = sc.total;
    ss::LineSum *sum = sc.sum;
    ss::LinePre *pre = sc.pre;
    ss::PlainArgs head = {hay, 0, ll.head_end, std::max<uint64_t>(ll.head_end, 1), sum, pre, o.begin, o.end, o.number, o.capacity, 0,
                          (uint32_t)delimiter, ss::kLinesSum};
    ss::PlainArgs tail = head;
    tail.begin = ll.tail_begin;
    tail.end = len;
    tail.part_bytes = std::max<uint64_t>(len - ll.tail_begin, 1);
    tail.part0 = blocks + 1;
    HIP_TRY(ss::launch_lines_plain(head, false, st));
    HIP_TRY(ss::launch_lines_plain(tail, false, st));
    ss::LineArgs la = {sum, pre, o.begin, o.end, o.number, o.capacity, ll.dlo, ll.dhi, ll.hshift, 1, (uint32_t)delimiter, ss::kLinesSum};
    if (!scan(ll.pr, ll.q, ll.mode, ll.one_byte, ll.shape, st, la, bound))
        return fail(SS_ERR_ARGUMENT, "no lines kernel for mode %d, window %d", ll.mode, ll.q);
    HIP_TRY(hipGetLastError());
    if (int rc = combine_parts(sc, len, o, emit, st, inv)) return rc;
    if (emit && inv) {
        // every part that closes a line without a match writes: the head too (it holds no match, so all of its lines are selected)
        la.mode = head.mode = tail.mode = ss::kLinesEmit;
        if (ll.head_end > 0) HIP_TRY(inv->plain(head, st));
        (void)inv->emit(ll.pr, ll.q, ll.mode, ll.one_byte, ll.shape, st, la, bound);
        HIP_TRY(hipGetLastError());
        if (ll.tail_begin < len) HIP_TRY(inv->plain(tail, st));
    } else if (emit) {
        la.mode = ss::kLinesEmit;
        (void)scan(ll.pr, ll.q, ll.mode, ll.one_byte, ll.shape, st, la, bound);
        HIP_TRY(hipGetLastError());
        if (ll.tail_begin < len) {              // (the head has nothing in front of it that could be pending)
            tail.mode = ss::kLinesEmit;
            HIP_TRY(ss::launch_lines_plain(tail, false, st));
        }
    }
    return SS_OK;
}

int check_args(const ss_searcher *s, const void *d_haystack, size_t len, int delimiter, const void *out)
{
    if (int rc = check_common_args(s, d_haystack, len, out)) return rc;
    if (delimiter < 0 || delimiter > 255) return fail(SS_ERR_ARGUMENT, "delimiter %d is not a byte (0 .. 255)", delimiter);
    return SS_OK;
}

// no line can match: an empty view, a needle longer than it, or one that holds the delimiter
bool no_line(const ss_searcher *s, size_t len, int delimiter)
{
    if (len == 0 || s->n > len) return true;
    return std::find(s->needle.begin(), s->needle.begin() + (long)s->n, (uint8_t)delimiter) != s->needle.begin() + (long)s->n;
}

// The answer that needs no launch, if there is one: no line matches - 0, or for an inverted call every line, which is the empty
// needle's pass (*every) unless the view is empty; the empty needle matches every line, so its inverse selects none.
bool settled(const ss_searcher *s, size_t len, int delimiter, const LinesInverted *inv, bool *every)
{
    *every = s->n == 0;
    if (!inv) return no_line(s, len, delimiter);
    if (len == 0 || s->n == 0) return true;
    *every = no_line(s, len, delimiter);
    return false;
}

int lines_blocking(ss::ScanLinesFn scan, const ss_searcher *s, const void *d_haystack, size_t len, int delimiter, void *hip_stream, const LinesOut &o,
                   uint64_t *lines, uint32_t bound, const LinesInverted *inv)
{
    SearchGate gate(s);                                  // set_filter* are refused while this call runs
    bool every = false;
    if (settled(s, len, delimiter, inv, &every)) { *lines = 0; return SS_OK; }
    if (every) inv = nullptr;
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    PerDevice *pd = nullptr;
    if (int rc = get_per_device(s, &pd)) return rc;
    ScratchLease lease;
    uint64_t *d_total = nullptr;
    if (int rc = enqueue_lines(scan, s, pd, d_haystack, len, delimiter, st, o, &lease, &d_total, bound, every, inv)) return rc;
    HIP_TRY(hipMemcpyAsync(lease.sc.h, d_total, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    lease.done = true;
    *lines = *lease.sc.h;
    return SS_OK;
}

}  // namespace

// (lines_host.hpp: `scan` is launch_scan_lines, or its case-folding twin for ss_nocase.hip)
int count_lines_device_with(ss::ScanLinesFn scan, const ss_searcher *s, const void *d_haystack, size_t len, int delimiter,
                            void *hip_stream, uint64_t *lines, uint32_t bound, const LinesInverted *inverted)
{
    if (int rc = check_args(s, d_haystack, len, delimiter, lines)) return rc;
    return lines_blocking(scan, s, d_haystack, len, delimiter, hip_stream, LinesOut{}, lines, bound, inverted);
}

int count_lines_device_async_with(ss::ScanLinesFn scan, const char *name, const ss_searcher *s, const void *d_haystack, size_t len,
                                  int delimiter, void *hip_stream, uint64_t *d_lines, uint32_t bound, const LinesInverted *inverted)
{
    if (int rc = check_args(s, d_haystack, len, delimiter, d_lines)) return rc;
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    if (stream_is_capturing(st))
        return fail(SS_ERR_ARGUMENT, "%s keeps scratch that later calls take over and cannot be captured into a hipGraph", name);
    SearchGate gate(s);
    PerDevice *pd = nullptr;
    if (int rc = get_per_device(s, &pd)) return rc;
    s->used_async.store(true, std::memory_order_release);
    bool every = false;
    if (settled(s, len, delimiter, inverted, &every)) {
        HIP_TRY(hipMemsetAsync(d_lines, 0, sizeof(uint64_t), st));
        return SS_OK;
    }
    if (every) inverted = nullptr;
    LinesOut o;
    o.d_total2 = d_lines;
    ScratchLease lease;
    uint64_t *d_total = nullptr;
    if (int rc = enqueue_lines(scan, s, pd, d_haystack, len, delimiter, st, o, &lease, &d_total, bound, every, inverted)) return rc;
    return lease.release_on(st);
}

int find_lines_device_with(ss::ScanLinesFn scan, const ss_searcher *s, const void *d_haystack, size_t len, int delimiter,
                           void *hip_stream, uint64_t *d_begin, uint64_t *d_end, uint64_t *d_number, uint64_t capacity, uint64_t *lines,
                           uint32_t bound, const LinesInverted *inverted)
{
    if (int rc = check_args(s, d_haystack, len, delimiter, lines)) return rc;
    LinesOut o;
    o.begin = d_begin;
    o.end = d_end;
    o.number = d_number;
    o.capacity = capacity;
    return lines_blocking(scan, s, d_haystack, len, delimiter, hip_stream, o, lines, bound, inverted);
}

}  // namespace ssh

using namespace ssh;

extern "C" {

int ss_count_lines_device(const ss_searcher *s, const void *d_haystack, size_t len, int delimiter, void *hip_stream, uint64_t *lines)
{
    return count_lines_device_with(ss::launch_scan_lines, s, d_haystack, len, delimiter, hip_stream, lines);
}

int ss_count_lines_device_async(const ss_searcher *s, const void *d_haystack, size_t len, int delimiter, void *hip_stream,
                                uint64_t *d_lines)
{
    return count_lines_device_async_with(ss::launch_scan_lines, "ss_count_lines_device_async", s, d_haystack, len, delimiter, hip_stream,
                                         d_lines);
}

int ss_find_lines_device(const ss_searcher *s, const void *d_haystack, size_t len, int delimiter, void *hip_stream, uint64_t *d_begin,
                         uint64_t *d_end, uint64_t *d_number, uint64_t capacity, uint64_t *lines)
{
    return find_lines_device_with(ss::launch_scan_lines, s, d_haystack, len, delimiter, hip_stream, d_begin, d_end, d_number, capacity,
                                  lines);
}

}  // extern "C"
