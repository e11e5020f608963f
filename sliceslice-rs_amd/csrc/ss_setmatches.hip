// ss_setmatches.hip - every occurrence of every needle of a set, counted per needle and listed as (offset, rank) pairs in ONE pass
// over the haystack (include/sliceslice_hip_setmatches.h): ss_needle_set_ranks, ss_count_set_device / _async and
// ss_find_all_set_device.  NOT in the other libraries: libsliceslice_hip_setmatches.so holds the needleset library's objects plus
// this file.
//
// A call cuts the view into parts of kSetPartBytes from the 16-byte aligned address at or below it, one workgroup each, as
// ss_needleset.hip does:
//   count   the outputs are zeroed on the stream, then set_all_kernel<kSetAllCount> adds into them.  The async form needs nothing
//           else and can be captured; the waiting form keeps the total in call-owned scratch and reads it back.
//   find    the count pass with one word per workgroup and no bins, the exclusive prefix of those words (prefix_kernel.hpp, one
//           workgroup), and set_all_kernel<kSetAllEmit> over the workgroups that hold one of the first `capacity` pairs, as
//           ss_find_all_device does it (ss_matches.hip).
#include "ss_internal.hpp"

#include "../../include/sliceslice_hip_setmatches.h"
#include "matches_scratch.hpp"
#include "needleset_host.hpp"
#include "prefix_kernel.hpp"
#include "setmatches_kernels.hpp"

namespace ss {

hipError_t launch_set_all(const SetAllArgs &a, int mode, hipStream_t st)
{
    const dim3 grid((unsigned)((a.ntiles + kSetTiles - 1) / kSetTiles)), block(kBlock);
    const bool fold = a.tv.fold != 0;
    if (mode == kSetAllCount) {
        if (fold) hipLaunchKernelGGL((set_all_kernel<kSetAllCount, true>), grid, block, 0, st, a);
        else hipLaunchKernelGGL((set_all_kernel<kSetAllCount, false>), grid, block, 0, st, a);
    } else {
        if (fold) hipLaunchKernelGGL((set_all_kernel<kSetAllEmit, true>), grid, block, 0, st, a);
        else hipLaunchKernelGGL((set_all_kernel<kSetAllEmit, false>), grid, block, 0, st, a);
    }
    return hipGetLastError();
}

hipError_t launch_set_prefix(const uint64_t *count, uint64_t n, uint64_t *rank, uint64_t *total, hipStream_t st)
{
    hipLaunchKernelGGL((prefix_kernel<uint64_t>), dim3(1), dim3(kPrefixThreads), 0, st, count, n, rank, total);
    return hipGetLastError();
}

}  // namespace ss

namespace ssh {
namespace {

// What all three scans refuse, and the argument block of the view.  `waits`: the call waits for its stream.
int set_all_args(const char *name, const ss_needle_set *set, const void *d_haystack, size_t len, unsigned how, bool waits, hipStream_t st,
                 ss::SetAllArgs *a)
{
    if (!set) return fail(SS_ERR_ARGUMENT, "%s: the set is NULL", name);
    if (len && !d_haystack) return fail(SS_ERR_ARGUMENT, "%s: haystack is NULL", name);
    if (how & (SS_BOUND_LINE | SS_CONTEXT_INVERT))
        return fail(SS_ERR_ARGUMENT, "%s: how = 0x%x holds SS_BOUND_LINE or SS_CONTEXT_INVERT; occurrences know no line and have no complement", name, how);
    if (how & ~(SS_BOUND_WORD | SS_BOUND_NOCASE)) return fail(SS_ERR_ARGUMENT, "%s: how = 0x%x holds bits other than SS_BOUND_WORD | SS_BOUND_NOCASE", name, how);
    if (((how & SS_BOUND_NOCASE) != 0) != (set->host.fold != 0))
        return fail(SS_ERR_ARGUMENT, "%s: how %s SS_BOUND_NOCASE, but the set was made %s SS_SET_NOCASE", name,
                    (how & SS_BOUND_NOCASE) ? "holds" : "does not hold", set->host.fold ? "with" : "without");
    if (set->host.every) return fail(SS_ERR_ARGUMENT, "%s: the set holds the empty needle, whose len + 1 occurrences belong to no scan", name);
    if (waits && stream_is_capturing(st)) return fail(SS_ERR_ARGUMENT, "%s waits for its stream and cannot be captured into a hipGraph", name);
    int dev = -1;
    HIP_TRY(hipGetDevice(&dev));
    if (dev != set->dev) return fail(SS_ERR_ARGUMENT, "%s: the set was made on device %d, the current device is %d", name, set->dev, dev);
    const uint8_t *hay = static_cast<const uint8_t *>(d_haystack);
    *a = ss::SetAllArgs{};
    a->mis = (uint64_t)(reinterpret_cast<uintptr_t>(hay) & 15);
    a->base = hay - a->mis;
    a->hay = hay;
    a->len = len;
    a->nchunks = (a->mis + len + 15) / 16;
    a->ntiles = (a->nchunks + ss::kSetTileChunks - 1) / ss::kSetTileChunks;
    a->tv = set->dev_view;
    a->tr = set->dev_ranks;
    a->how = how & SS_BOUND_WORD;
    if ((a->ntiles + ss::kSetTiles - 1) / ss::kSetTiles > 0x7fffffffull)
        return fail(SS_ERR_ARGUMENT, "%s: a haystack of %zu bytes needs more than 2^31 - 1 workgroups", name, len);
    return SS_OK;
}

}  // namespace
}  // namespace ssh

using namespace ssh;

extern "C" {

int ss_needle_set_ranks(const ss_needle_set *set, uint32_t *ranks)
{
    if (!set || !ranks) return fail(SS_ERR_ARGUMENT, "NULL argument");
    std::copy(set->host.rank_of.begin(), set->host.rank_of.end(), ranks);
    return SS_OK;
}

int ss_count_set_device_async(const ss_needle_set *set, const void *d_haystack, size_t len, unsigned how, void *hip_stream,
                              uint64_t *d_counts, uint64_t *d_total)
{
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    if (!d_counts && !d_total) return fail(SS_ERR_ARGUMENT, "ss_count_set_device_async: d_counts and d_total are both NULL");
    ss::SetAllArgs a;
    if (int rc = set_all_args("ss_count_set_device_async", set, d_haystack, len, how, false, st, &a)) return rc;
    if (d_counts) HIP_TRY(hipMemsetAsync(d_counts, 0, (size_t)set->host.distinct * sizeof(uint64_t), st));
    if (d_total) HIP_TRY(hipMemsetAsync(d_total, 0, sizeof(uint64_t), st));
    if (len == 0) return SS_OK;
    a.counts = d_counts;
    a.total = d_total;
    HIP_TRY(ss::launch_set_all(a, ss::kSetAllCount, st));
    return SS_OK;
}

int ss_count_set_device(const ss_needle_set *set, const void *d_haystack, size_t len, unsigned how, void *hip_stream, uint64_t *d_counts,
                        uint64_t *total)
{
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    if (!total) return fail(SS_ERR_ARGUMENT, "ss_count_set_device: total is NULL");
    ss::SetAllArgs a;
    if (int rc = set_all_args("ss_count_set_device", set, d_haystack, len, how, true, st, &a)) return rc;
    ScratchLease lease;
    if (len != 0)
        if (int rc = take_scratch(set->dev, sizeof(uint64_t), &lease.sc, st)) return rc;
    if (d_counts) HIP_TRY(hipMemsetAsync(d_counts, 0, (size_t)set->host.distinct * sizeof(uint64_t), st));
    if (len == 0) {
        if (d_counts) HIP_TRY(hipStreamSynchronize(st));
        *total = 0;
        return SS_OK;
    }
    a.counts = d_counts;
    a.total = reinterpret_cast<uint64_t *>(lease.sc.d);
    HIP_TRY(hipMemsetAsync(a.total, 0, sizeof(uint64_t), st));
    HIP_TRY(ss::launch_set_all(a, ss::kSetAllCount, st));
    HIP_TRY(hipMemcpyAsync(lease.sc.h, a.total, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    lease.done = true;
    *total = *lease.sc.h;
    return SS_OK;
}

int ss_find_all_set_device(const ss_needle_set *set, const void *d_haystack, size_t len, unsigned how, void *hip_stream, uint64_t *d_offsets,
                           uint32_t *d_ranks, uint64_t capacity, uint64_t *total)
{
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    if (!total) return fail(SS_ERR_ARGUMENT, "ss_find_all_set_device: total is NULL");
    ss::SetAllArgs a;
    if (int rc = set_all_args("ss_find_all_set_device", set, d_haystack, len, how, true, st, &a)) return rc;
    if (len == 0) {
        *total = 0;
        return SS_OK;
    }
    const uint64_t parts = (a.ntiles + ss::kSetTiles - 1) / ss::kSetTiles;
    // [total u64][rank u64 x parts][pairs u64 x parts]
    ScratchLease lease;
    if (int rc = take_scratch(set->dev, 8 + parts * 16, &lease.sc, st)) return rc;
    uint64_t *d_total = reinterpret_cast<uint64_t *>(lease.sc.d);
    uint64_t *d_rank = d_total + 1;
    a.wg = d_rank + parts;
    HIP_TRY(ss::launch_set_all(a, ss::kSetAllCount, st));
    HIP_TRY(ss::launch_set_prefix(a.wg, parts, d_rank, d_total, st));
    if (capacity != 0 && (d_offsets || d_ranks)) {
        a.wg_rank = d_rank;
        a.offsets = d_offsets;
        a.ranks = d_ranks;
        a.capacity = capacity;
        HIP_TRY(ss::launch_set_all(a, ss::kSetAllEmit, st));
    }
    HIP_TRY(hipMemcpyAsync(lease.sc.h, d_total, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    lease.done = true;
    *total = *lease.sc.h;
    return SS_OK;
}

}  // extern "C"
