// ss_needleset.hip - the lines that match any of many needles, selected in ONE pass over the haystack
// (include/sliceslice_hip_needleset.h): ss_needle_set_new / _free / _info, ss_count_lines_set_device and ss_find_lines_set_device.
// NOT in the other libraries: libsliceslice_hip_needleset.so holds the anyof library's objects plus this file.
//
// A set is its tables (needleset_tables.hpp), built on the host at construction and copied into ONE device allocation.  A call
// cuts the view into parts of kSetPartBytes from the 16-byte aligned address at or below it, one workgroup each:
//   count   set_scan_kernel<kSetSum> leaves a LineSum per part; lines_chunk_kernel and lines_combine_kernel as ss_lines.hip
//           launches them; with SS_CONTEXT_INVERT lines_total_inverted_kernel behind them (delimiters - matching lines, from the
//           same sums).  No census and no union.
//   find    before == after == 0: the states are spread back over the parts and set_scan_kernel<kSetEmit / kSetEmitInv> writes
//           the records into the caller's arrays; `kind` is one memset.  With context: the count first, ONE temporary buffer of
//           8 bytes per selected line, the emit pass with `number` only into it, ss_lines_around_device on it.
// A set that holds the empty needle selects every line: lines_plain_kernel in its EVERY form in place of the scan.
#include "ss_internal.hpp"

#include "../../include/sliceslice_hip_needleset.h"
#include "inverted_launch.hpp"
#include "matches_scratch.hpp"
#include "needleset_host.hpp"
#include "needleset_kernels.hpp"

#include <new>

namespace ss {

hipError_t launch_set_scan(const SetArgs &sa, int mode, hipStream_t st)
{
    const dim3 grid((unsigned)((sa.ntiles + kSetTiles - 1) / kSetTiles)), block(kBlock);
    const bool fold = sa.tv.fold != 0;
    if (mode == kSetSum) {
        if (fold) hipLaunchKernelGGL((set_scan_kernel<kSetSum, true>), grid, block, 0, st, sa);
        else hipLaunchKernelGGL((set_scan_kernel<kSetSum, false>), grid, block, 0, st, sa);
    } else if (mode == kSetEmit) {
        if (fold) hipLaunchKernelGGL((set_scan_kernel<kSetEmit, true>), grid, block, 0, st, sa);
        else hipLaunchKernelGGL((set_scan_kernel<kSetEmit, false>), grid, block, 0, st, sa);
    } else {
        if (fold) hipLaunchKernelGGL((set_scan_kernel<kSetEmitInv, true>), grid, block, 0, st, sa);
        else hipLaunchKernelGGL((set_scan_kernel<kSetEmitInv, false>), grid, block, 0, st, sa);
    }
    return hipGetLastError();
}

}  // namespace ss

namespace ssh {
namespace {

constexpr uint64_t kPlainPart = 64 * 1024;          // bytes per workgroup of the pass of a set that holds the empty needle
constexpr unsigned kHowBits = SS_BOUND_WORD | SS_BOUND_LINE | SS_BOUND_NOCASE | SS_CONTEXT_INVERT;

size_t pad16(size_t n) { return (n + 15) & ~(size_t)15; }

// [total, 32 bytes][LineSum x parts][LinePre x parts][LineSum x chunks][LinePre x chunks], as ss_lines.hip lays it out
struct SetScratch {
    uint64_t parts = 0, chunks = 0;
    uint64_t *total = nullptr;
    ss::LineSum *sum = nullptr, *csum = nullptr;
    ss::LinePre *pre = nullptr, *cpre = nullptr;
};

int take_set_scratch(int dev, uint64_t parts, hipStream_t st, ScratchLease *lease, SetScratch *out)
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

// temporary device memory of a find call with context, returned on every way out
struct DeviceWords {
    uint64_t *d = nullptr;
    ~DeviceWords() { if (d) (void)hipFree(d); }
    int take(uint64_t words, const char *name)
    {
        if (words > SIZE_MAX / sizeof(uint64_t)) return fail(SS_ERR_NOMEM, "%s: %llu selected lines are too many to number", name, (unsigned long long)words);
        const hipError_t e = hipMalloc(reinterpret_cast<void **>(&d), words * sizeof(uint64_t));
        if (e == hipSuccess) return SS_OK;
        (void)hipGetLastError();
        d = nullptr;
        return fail(e == hipErrorOutOfMemory ? SS_ERR_NOMEM : SS_ERR_HIP, "%s: %llu bytes for the numbers of the selected lines: %s", name,
                    (unsigned long long)(words * sizeof(uint64_t)), hipGetErrorString(e));
    }
};

// The passes of one call over its parts: the scan of the set, or - for a set that holds the empty needle - the plain pass that
// selects every line.
struct Passes {
    bool every = false, invert = false;
    ss::SetArgs sa = {};
    ss::PlainArgs pa = {};
    SetScratch sc;
    uint64_t len = 0;

    int sum(hipStream_t st)
    {
        if (every) {
            pa.mode = ss::kLinesSum;
            HIP_TRY(ss::launch_lines_plain(pa, true, st));
        } else {
            HIP_TRY(ss::launch_set_scan(sa, ss::kSetSum, st));
        }
        HIP_TRY(ss::launch_lines_chunks(sc.sum, sc.parts, sc.csum, sc.cpre, sc.pre, false, st));
        return SS_OK;
    }
    // the total, the record of an unterminated last line below the capacity and - emit - the records of every other selected line
    int combine(uint64_t *begin, uint64_t *end, uint64_t *number, uint64_t capacity, hipStream_t st)
    {
        const bool emit = capacity != 0 && (begin || end || number);
        ss::CombineArgs ca = {sc.csum, sc.chunks, sc.cpre, sc.total, nullptr, len, begin, end, number, emit && !invert ? capacity : 0};
        HIP_TRY(ss::launch_lines_combine(ca, st));
        if (invert) {
            ca.capacity = emit ? capacity : 0;
            HIP_TRY(ss::launch_lines_total_inverted(ca, st));
        }
        if (!emit) return SS_OK;
        HIP_TRY(ss::launch_lines_chunks(sc.sum, sc.parts, sc.csum, sc.cpre, sc.pre, true, st));
        if (every) {
            pa.mode = ss::kLinesEmit;
            pa.out_begin = begin;
            pa.out_end = end;
            pa.out_number = number;
            pa.capacity = capacity;
            HIP_TRY(ss::launch_lines_plain(pa, true, st));
        } else {
            sa.begin = begin;
            sa.end = end;
            sa.number = number;
            sa.capacity = capacity;
            HIP_TRY(ss::launch_set_scan(sa, invert ? ss::kSetEmitInv : ss::kSetEmit, st));
        }
        return SS_OK;
    }
};

// Both line calls.  `find`: records and context are wanted (else the five output arguments are unused).
int lines_set(const char *name, bool find, const ss_needle_set *set, const void *d_haystack, size_t len, int delimiter, unsigned how,
              uint64_t before, uint64_t after, void *hip_stream, uint64_t *d_begin, uint64_t *d_end, uint64_t *d_number, uint8_t *d_kind,
              uint64_t capacity, uint64_t *lines, uint64_t *selected)
{
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    if (!set || !lines || !selected) return fail(SS_ERR_ARGUMENT, "NULL argument");
    if (len && !d_haystack) return fail(SS_ERR_ARGUMENT, "haystack is NULL");
    if (delimiter < 0 || delimiter > 255) return fail(SS_ERR_ARGUMENT, "delimiter %d is not a byte (0 .. 255)", delimiter);
    if (how & ~kHowBits)
        return fail(SS_ERR_ARGUMENT, "%s: how = 0x%x holds bits other than SS_BOUND_WORD | SS_BOUND_LINE | SS_BOUND_NOCASE | SS_CONTEXT_INVERT", name, how);
    if (((how & SS_BOUND_NOCASE) != 0) != (set->host.fold != 0))
        return fail(SS_ERR_ARGUMENT, "%s: how %s SS_BOUND_NOCASE, but the set was made %s SS_SET_NOCASE", name,
                    (how & SS_BOUND_NOCASE) ? "holds" : "does not hold", set->host.fold ? "with" : "without");
    const unsigned bound = how & (SS_BOUND_WORD | SS_BOUND_LINE);
    if (bound == (SS_BOUND_WORD | SS_BOUND_LINE)) return fail(SS_ERR_ARGUMENT, "%s: SS_BOUND_WORD and SS_BOUND_LINE exclude each other", name);
    if (bound && set->host.every)
        return fail(SS_ERR_ARGUMENT, "%s: the set holds the empty needle, which has no whole-word or whole-line form", name);
    if (stream_is_capturing(st)) return fail(SS_ERR_ARGUMENT, "%s waits for its stream and cannot be captured into a hipGraph", name);
    int dev = -1;
    HIP_TRY(hipGetDevice(&dev));
    if (dev != set->dev) return fail(SS_ERR_ARGUMENT, "%s: the set was made on device %d, the current device is %d", name, set->dev, dev);

    Passes ps;
    ps.every = set->host.every != 0;
    ps.invert = (how & SS_CONTEXT_INVERT) != 0;
    ps.len = len;
    if (len == 0 || (ps.every && ps.invert)) {
        *lines = 0;
        *selected = 0;
        return SS_OK;
    }
    const uint8_t *hay = static_cast<const uint8_t *>(d_haystack);
    uint64_t parts;
    if (ps.every) {
        parts = (len + kPlainPart - 1) / kPlainPart;
    } else {
        ss::SetArgs &sa = ps.sa;
        sa.mis = (uint64_t)(reinterpret_cast<uintptr_t>(hay) & 15);
        sa.base = hay - sa.mis;
        sa.hay = hay;
        sa.len = len;
        sa.nchunks = (sa.mis + len + 15) / 16;
        sa.ntiles = (sa.nchunks + ss::kSetTileChunks - 1) / ss::kSetTileChunks;
        sa.tv = set->dev_view;
        sa.delim = (uint32_t)delimiter;
        sa.how = bound;
        parts = (sa.ntiles + ss::kSetTiles - 1) / ss::kSetTiles;
    }
    if (parts > 0x7fffffffull)
        return fail(SS_ERR_ARGUMENT, "a haystack of %zu bytes needs %llu workgroups; a grid holds 2^31 - 1", len, (unsigned long long)parts);
    ScratchLease lease;
    if (int rc = take_set_scratch(dev, parts, st, &lease, &ps.sc)) return rc;
    ps.sa.sum = ps.sc.sum;
    ps.sa.pre = ps.sc.pre;
    ps.pa = ss::PlainArgs{hay, 0, len, kPlainPart, ps.sc.sum, ps.sc.pre, nullptr, nullptr, nullptr, 0, 0, (uint32_t)delimiter, ss::kLinesSum};

    const bool context = find && (before != 0 || after != 0);
    if (int rc = ps.sum(st)) return rc;
    if (find && !context) {
        if (int rc = ps.combine(d_begin, d_end, d_number, capacity, st)) return rc;
    } else {
        if (int rc = ps.combine(nullptr, nullptr, nullptr, 0, st)) return rc;
    }
    HIP_TRY(hipMemcpyAsync(lease.sc.h, ps.sc.total, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    const uint64_t total = *lease.sc.h;
    if (!context) {
        if (find && d_kind && capacity != 0 && total != 0) {
            HIP_TRY(hipMemsetAsync(d_kind, 1, (size_t)(total < capacity ? total : capacity), st));
            HIP_TRY(hipStreamSynchronize(st));
        }
        lease.done = true;
        *lines = total;
        *selected = total;
        return SS_OK;
    }
    if (total == 0) {
        lease.done = true;
        *lines = 0;
        *selected = 0;
        return SS_OK;
    }
    // the selected numbers, all of them, then the primitive of sliceslice_hip_context.h (it waits for the stream)
    DeviceWords numbers;
    if (int rc = numbers.take(total, name)) {
        lease.done = true;
        return rc;
    }
    if (int rc = ps.combine(nullptr, nullptr, numbers.d, total, st)) return rc;
    uint64_t printed = 0;
    if (int rc = ss_lines_around_device(set->anchor, d_haystack, len, delimiter, numbers.d, total, before, after, hip_stream, d_begin, d_end,
                                        d_number, d_kind, capacity, &printed)) {
        (void)hipStreamSynchronize(st);                 // (the buffer is freed on the way out)
        return rc;
    }
    lease.done = true;
    *lines = printed;
    *selected = total;
    return SS_OK;
}

}  // namespace
}  // namespace ssh

using namespace ssh;

extern "C" {

int ss_needle_set_new(const void *const *needles, const size_t *lens, uint32_t count, unsigned flags, ss_needle_set **out)
{
    if (!needles || !lens || !out) return fail(SS_ERR_ARGUMENT, "NULL argument");
    if (count == 0) return fail(SS_ERR_ARGUMENT, "ss_needle_set_new: no needles");
    if (count > SS_ANYOF_MAX_NEEDLES)
        return fail(SS_ERR_ARGUMENT, "ss_needle_set_new: %u needles; a set takes %u", count, (unsigned)SS_ANYOF_MAX_NEEDLES);
    if (flags & ~SS_SET_NOCASE) return fail(SS_ERR_ARGUMENT, "ss_needle_set_new: flags = 0x%x holds bits other than SS_SET_NOCASE", flags);
    uint64_t bytes = 0;
    for (uint32_t k = 0; k < count; ++k) {
        if (lens[k] != 0 && !needles[k]) return fail(SS_ERR_ARGUMENT, "ss_needle_set_new: needles[%u] is NULL and lens[%u] is %zu", k, k, lens[k]);
        if (lens[k] >= (1ull << 32) || (bytes += lens[k]) >= (1ull << 32))
            return fail(SS_ERR_ARGUMENT, "ss_needle_set_new: the needles hold 2^32 bytes or more");
    }
    ss_needle_set *set = new (std::nothrow) ss_needle_set;
    if (!set) return fail(SS_ERR_NOMEM, "ss_needle_set_new: out of memory");
    struct Guard {
        ss_needle_set *s;
        ~Guard() { if (s) ss_needle_set_free(s); }
    } guard{set};
    try {
        if (ss::set_build(needles, lens, count, (flags & SS_SET_NOCASE) != 0, &set->host) != ss::kSetBuilt)
            return fail(SS_ERR_ARGUMENT, "ss_needle_set_new: the needles hold 2^32 bytes or more");
    } catch (const std::bad_alloc &) {
        return fail(SS_ERR_NOMEM, "ss_needle_set_new: out of memory");
    }
    HIP_TRY(hipGetDevice(&set->dev));
    if (int rc = ss_searcher_new(reinterpret_cast<const uint8_t *>("a"), 1, &set->anchor)) return rc;
    const ss::SetTables &t = set->host;
    const size_t o_bp = 0, o_b1 = o_bp + pad16(t.bp.size() * 4), o_bucket = o_b1 + pad16(t.b1.size() * 4),
                 o_entry = o_bucket + pad16(t.bucket.size() * 4), o_blob = o_entry + pad16(t.entry.size() * sizeof(ss::SetEntry)),
                 o_rank1 = o_blob + pad16(t.blob.size() + 1), o_key2 = o_rank1 + pad16(t.rank1.size() * 4),
                 o_rank2 = o_key2 + pad16(t.key2.size() * 4 + 4), o_erank = o_rank2 + pad16(t.rank2.size() * 4 + 4),
                 o_slot = o_erank + pad16(t.erank.size() * 4 + 4), o_hot = o_slot + pad16(t.slot.size() * 4 + 4),
                 size = o_hot + pad16(t.hot.size() * 4 + 4);
    const hipError_t e = hipMalloc(reinterpret_cast<void **>(&set->d_mem), size);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        set->d_mem = nullptr;
        return fail(e == hipErrorOutOfMemory ? SS_ERR_NOMEM : SS_ERR_HIP, "ss_needle_set_new: %zu bytes for the tables: %s", size, hipGetErrorString(e));
    }
    HIP_TRY(hipMemcpy(set->d_mem + o_bp, t.bp.data(), t.bp.size() * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(set->d_mem + o_b1, t.b1.data(), t.b1.size() * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(set->d_mem + o_bucket, t.bucket.data(), t.bucket.size() * 4, hipMemcpyHostToDevice));
    if (!t.entry.empty()) HIP_TRY(hipMemcpy(set->d_mem + o_entry, t.entry.data(), t.entry.size() * sizeof(ss::SetEntry), hipMemcpyHostToDevice));
    if (!t.blob.empty()) HIP_TRY(hipMemcpy(set->d_mem + o_blob, t.blob.data(), t.blob.size(), hipMemcpyHostToDevice));
    // the side tables of needle identity (sliceslice_hip_setmatches.h), behind the blob
    auto up = [&](size_t at, const std::vector<uint32_t> &v) {
        return v.empty() ? hipSuccess : hipMemcpy(set->d_mem + at, v.data(), v.size() * 4, hipMemcpyHostToDevice);
    };
    HIP_TRY(up(o_rank1, t.rank1));
    HIP_TRY(up(o_key2, t.key2));
    HIP_TRY(up(o_rank2, t.rank2));
    HIP_TRY(up(o_erank, t.erank));
    HIP_TRY(up(o_slot, t.slot));
    HIP_TRY(up(o_hot, t.hot));
    auto words = [&](size_t at) { return reinterpret_cast<const uint32_t *>(set->d_mem + at); };
    set->dev_ranks = ss::SetRanks{words(o_rank1), words(o_key2), words(o_rank2), words(o_erank), words(o_slot), words(o_hot),
                                  (uint32_t)t.key2.size(), (uint32_t)t.hot.size()};
    set->dev_view = ss::SetView{reinterpret_cast<const uint32_t *>(set->d_mem + o_b1), reinterpret_cast<const uint32_t *>(set->d_mem + o_bp),
                                reinterpret_cast<const uint32_t *>(set->d_mem + o_bucket), reinterpret_cast<const ss::SetEntry *>(set->d_mem + o_entry),
                                set->d_mem + o_blob, t.fold, t.one_byte != 0 ? 1u : 0u};
    guard.s = nullptr;
    *out = set;
    return SS_OK;
}

void ss_needle_set_free(ss_needle_set *set)
{
    if (!set) return;
    if (set->d_mem) (void)hipFree(set->d_mem);
    if (set->anchor) ss_searcher_free(set->anchor);
    delete set;
}

int ss_needle_set_info(const ss_needle_set *set, ss_needle_set_stats *stats)
{
    if (!set || !stats) return fail(SS_ERR_ARGUMENT, "NULL argument");
    const ss::SetTables &t = set->host;
    *stats = ss_needle_set_stats{t.needles, t.distinct, t.blob.size(), t.one_byte, t.two_byte, t.keys, t.largest_bucket, t.fold};
    return SS_OK;
}

int ss_count_lines_set_device(const ss_needle_set *set, const void *d_haystack, size_t len, int delimiter, unsigned how, void *hip_stream,
                              uint64_t *lines)
{
    uint64_t unused = 0;
    return lines_set("ss_count_lines_set_device", false, set, d_haystack, len, delimiter, how, 0, 0, hip_stream, nullptr, nullptr, nullptr,
                     nullptr, 0, lines, &unused);
}

int ss_find_lines_set_device(const ss_needle_set *set, const void *d_haystack, size_t len, int delimiter, unsigned how, uint64_t before,
                             uint64_t after, void *hip_stream, uint64_t *d_begin, uint64_t *d_end, uint64_t *d_number, uint8_t *d_kind,
                             uint64_t capacity, uint64_t *lines, uint64_t *selected)
{
    return lines_set("ss_find_lines_set_device", true, set, d_haystack, len, delimiter, how, before, after, hip_stream, d_begin, d_end,
                     d_number, d_kind, capacity, lines, selected);
}

}  // extern "C"
