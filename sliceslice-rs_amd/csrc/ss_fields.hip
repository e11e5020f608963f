// ss_fields.hip - fields first .. last of every line, located on the device (include/sliceslice_hip_fields.h has THE RULE and the
// language): ss_fields_new / _free / _info, ss_fields_parse, ss_count_fields_device and ss_find_fields_device.  NOT in the other
// libraries: libsliceslice_hip_fields.so holds the rewrite library's objects plus this file.
//
// A handle is host memory alone.  A call builds the set its kernels test - EACH: the separators without the delimiter, MERGE: every
// byte that is neither - with its ranges' constants, runs one pass that leaves a summary per workgroup, the carry kernel over the
// summaries and, for a find with room for records, the same grid again.
#include "ss_internal.hpp"

#include "../../include/sliceslice_hip_fields.h"
#include "classes_host.hpp"
#include "fields_host.hpp"
#include "fields_kernels.hpp"
#include "matches_scratch.hpp"

#include <new>

struct ss_fields {
    uint64_t set[4];
    int mode;
    uint64_t first, last;
    unsigned flags;
    int dev;
};

namespace ss {

hipError_t launch_fields(const FieldsArgs &a, int mode, hipStream_t st)
{
    const dim3 grid((unsigned)((a.r.m.ntiles + kSetTiles - 1) / kSetTiles)), block(kBlock);
    if (mode == kFieldsSum) hipLaunchKernelGGL((fields_kernel<kFieldsSum>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((fields_kernel<kFieldsEmit>), grid, block, 0, st, a);
    return hipGetLastError();
}

hipError_t launch_fields_carry(const FieldsCarryArgs &a, hipStream_t st)
{
    hipLaunchKernelGGL(fields_carry_kernel, dim3(1), dim3(kFieldsCarryChunk), 0, st, a);
    return hipGetLastError();
}

}  // namespace ss

namespace ssh {
namespace {

// What both scans refuse, and the argument block of the view and the set.
int fields_args(const char *name, const ss_fields *p, const void *d_haystack, size_t len, int delimiter, hipStream_t st, ss::FieldsArgs *fa)
{
    if (!p) return fail(SS_ERR_ARGUMENT, "%s: fields is NULL", name);
    if (len && !d_haystack) return fail(SS_ERR_ARGUMENT, "%s: haystack is NULL", name);
    if (delimiter < 0 || delimiter > 255) return fail(SS_ERR_ARGUMENT, "%s: delimiter %d is not a byte (0 .. 255)", name, delimiter);
    if (classes::set_has(p->set, (unsigned)delimiter) && classes::set_size(p->set) == 1)
        return fail(SS_ERR_ARGUMENT, "%s: the set is only the delimiter 0x%02x, which never separates: there is no separator", name, delimiter);
    if (stream_is_capturing(st)) return fail(SS_ERR_ARGUMENT, "%s waits for its stream and cannot be captured into a hipGraph", name);
    int dev = -1;
    HIP_TRY(hipGetDevice(&dev));
    if (dev != p->dev) return fail(SS_ERR_ARGUMENT, "%s: the handle was made on device %d, the current device is %d", name, p->dev, dev);
    const uint8_t *hay = static_cast<const uint8_t *>(d_haystack);
    *fa = ss::FieldsArgs{};
    ss::RunsArgs *ra = &fa->r;
    ss::MaskedArgs *a = &ra->m;
    a->mis = (uint64_t)(reinterpret_cast<uintptr_t>(hay) & 15);
    a->base = hay - a->mis;
    a->hay = hay;
    a->len = len;
    a->nchunks = (a->mis + len + 15) / 16;
    a->ntiles = (a->nchunks + ss::kSetTileChunks - 1) / ss::kSetTileChunks;
    if ((a->ntiles + ss::kSetTiles - 1) / ss::kSetTiles > 0x7fffffffull)
        return fail(SS_ERR_ARGUMENT, "%s: a haystack of %zu bytes needs more than 2^31 - 1 workgroups", name, len);
    // the set the kernels test: the separators (EACH) or the field bytes (MERGE), never the delimiter
    uint64_t set[4];
    for (int k = 0; k < 4; ++k) set[k] = p->mode == SS_FIELDS_MERGE ? ~p->set[k] : p->set[k];
    set[delimiter >> 6] &= ~(1ull << (delimiter & 63));
    uint8_t lo[ss::kRunsMaxRanges] = {0, 0, 0, 0}, hi[ss::kRunsMaxRanges] = {0, 0, 0, 0};
    const unsigned nranges = ss::runs_ranges(set, lo, hi, ss::kRunsMaxRanges);
    ra->nranges = nranges <= (unsigned)ss::kRunsMaxRanges ? nranges : 0u;       // (0: the bitmap, also for an empty set of field bytes)
    for (int r = 0; r < ss::kRunsMaxRanges; ++r) ra->rg[r] = ss::runs_range(lo[r], hi[r]);
    for (int k = 0; k < 4; ++k) {
        ra->bits[2 * k] = (uint32_t)set[k];
        ra->bits[2 * k + 1] = (uint32_t)(set[k] >> 32);
    }
    ra->min_len = 1;
    ra->max_len = 0;
    ra->look = 1;
    ra->simple = 1;                                                             // every begin and end of a run of field bytes counts
    fa->first = p->first;
    fa->last = p->last;
    fa->merge = p->mode == SS_FIELDS_MERGE ? 1u : 0u;
    fa->delim = (uint32_t)delimiter;
    return SS_OK;
}

// Pass 1 and the carry kernel; totals[0 .. 2] = record begins, record ends, lines come back in host memory.
// [totals, 32 bytes][FieldsSum x parts][FieldsPre x parts]
int fields_scan(const ss_fields *p, ss::FieldsArgs &fa, hipStream_t st, ScratchLease &lease, uint64_t *d_totals_out[1])
{
    const uint64_t parts = (fa.r.m.ntiles + ss::kSetTiles - 1) / ss::kSetTiles;
    if (int rc = take_scratch(p->dev, 32 + parts * (sizeof(ss::FieldsSum) + sizeof(ss::FieldsPre)), &lease.sc, st)) return rc;
    uint64_t *d_totals = reinterpret_cast<uint64_t *>(lease.sc.d);
    ss::FieldsSum *sum = reinterpret_cast<ss::FieldsSum *>(lease.sc.d + 32);
    ss::FieldsPre *pre = reinterpret_cast<ss::FieldsPre *>(sum + parts);
    fa.sum = sum;
    fa.pre = pre;
    HIP_TRY(ss::launch_fields(fa, ss::kFieldsSum, st));
    const ss::FieldsCarryArgs ca = {sum, pre, parts, fa.first, fa.last, fa.merge, fa.keep, d_totals};
    HIP_TRY(ss::launch_fields_carry(ca, st));
    d_totals_out[0] = d_totals;
    return SS_OK;
}

}  // namespace
}  // namespace ssh

using namespace ssh;

extern "C" {

int ss_fields_parse(const char *text, uint64_t *first, uint64_t *last)
{
    if (!text || !first || !last) return fail(SS_ERR_ARGUMENT, "ss_fields_parse: NULL argument");
    fields::ParseError err = {0, nullptr};
    uint64_t lo = 0, hi = 0;
    if (!fields::parse_fields(text, &lo, &hi, &err)) return fail(SS_ERR_ARGUMENT, "ss_fields_parse: column %zu: %s", err.column, err.what);
    *first = lo;
    *last = hi;
    return SS_OK;
}

int ss_fields_new(const uint64_t *set, int mode, uint64_t first, uint64_t last, unsigned flags, ss_fields **out)
{
    if (!out || !set) return fail(SS_ERR_ARGUMENT, "ss_fields_new: NULL argument");
    if (classes::set_size(set) == 0) return fail(SS_ERR_ARGUMENT, "ss_fields_new: the set is empty");
    if (const char *why = fields::check_selection(mode, first, last, flags)) return fail(SS_ERR_ARGUMENT, "ss_fields_new: %s", why);
    ss_fields *p = new (std::nothrow) ss_fields;
    if (!p) return fail(SS_ERR_NOMEM, "ss_fields_new: out of memory");
    for (int k = 0; k < 4; ++k) p->set[k] = set[k];
    p->mode = mode;
    p->first = first;
    p->last = last;
    p->flags = flags;
    const hipError_t e = hipGetDevice(&p->dev);
    if (e != hipSuccess) {
        delete p;
        return fail(SS_ERR_HIP, "ss_fields_new: %s", hipGetErrorString(e));
    }
    *out = p;
    return SS_OK;
}

void ss_fields_free(ss_fields *p) { delete p; }

int ss_fields_info(const ss_fields *p, int delimiter, ss_fields_stats *stats)
{
    if (!p || !stats) return fail(SS_ERR_ARGUMENT, "ss_fields_info: NULL argument");
    if (delimiter > 255) return fail(SS_ERR_ARGUMENT, "ss_fields_info: delimiter %d is not a byte (0 .. 255)", delimiter);
    const ss_fields_stats s = {(uint64_t)p->mode, p->first, p->last, p->flags, classes::set_size(p->set),
                               delimiter >= 0 && classes::set_has(p->set, (unsigned)delimiter) ? 1u : 0u};
    *stats = s;
    return SS_OK;
}

int ss_count_fields_device(const ss_fields *p, const void *d_haystack, size_t len, int delimiter, void *hip_stream, uint64_t *lines_selected,
                           uint64_t *lines_total)
{
    const char *name = "ss_count_fields_device";
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    if (!lines_selected || !lines_total) return fail(SS_ERR_ARGUMENT, "%s: lines_selected or lines_total is NULL", name);
    ss::FieldsArgs fa;
    if (int rc = fields_args(name, p, d_haystack, len, delimiter, st, &fa)) return rc;
    if (len == 0) {
        *lines_selected = 0;
        *lines_total = 0;
        return SS_OK;
    }
    fa.keep = 0;                                                                // the selected lines are the begins without KEEP_SHORT
    ScratchLease lease;
    uint64_t *d_totals[1] = {nullptr};
    if (int rc = fields_scan(p, fa, st, lease, d_totals)) return rc;
    uint64_t totals[3] = {0, 0, 0};
    HIP_TRY(hipMemcpyAsync(totals, d_totals[0], sizeof(totals), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    lease.done = true;
    *lines_selected = totals[0];
    *lines_total = totals[2];
    return SS_OK;
}

int ss_find_fields_device(const ss_fields *p, const void *d_haystack, size_t len, int delimiter, void *hip_stream, uint64_t *d_begin,
                          uint64_t *d_end, uint64_t *d_number, uint64_t capacity, uint64_t *total)
{
    const char *name = "ss_find_fields_device";
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    if (!total) return fail(SS_ERR_ARGUMENT, "%s: total is NULL", name);
    if (capacity && !d_begin && !d_end && !d_number)
        return fail(SS_ERR_ARGUMENT, "%s: all three arrays are NULL with a capacity of %llu", name, (unsigned long long)capacity);
    ss::FieldsArgs fa;
    if (int rc = fields_args(name, p, d_haystack, len, delimiter, st, &fa)) return rc;
    if (len == 0) {
        *total = 0;
        return SS_OK;
    }
    fa.keep = (p->flags & SS_FIELDS_KEEP_SHORT) ? 1u : 0u;
    ScratchLease lease;
    uint64_t *d_totals[1] = {nullptr};
    if (int rc = fields_scan(p, fa, st, lease, d_totals)) return rc;
    if (capacity != 0) {
        fa.out_b = d_begin;
        fa.out_e = d_end;
        fa.out_n = d_number;
        fa.r.m.capacity = capacity;
        HIP_TRY(ss::launch_fields(fa, ss::kFieldsEmit, st));
    }
    uint64_t totals[3] = {0, 0, 0};
    HIP_TRY(hipMemcpyAsync(totals, d_totals[0], sizeof(totals), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    lease.done = true;
    if (totals[0] != totals[1])
        return fail(SS_ERR_ARGUMENT, "%s: the haystack changed under the call (%llu begins, %llu ends)", name, (unsigned long long)totals[0],
                    (unsigned long long)totals[1]);
    *total = totals[0];
    return SS_OK;
}

}  // extern "C"
