// ss_groups.hip - equal keys grouped and counted on the device (include/sliceslice_hip_groups.h has THE RULE):
// ss_group_ranges_device, ss_group_runs_device, ss_group_lines_device and ss_groups_scratch_bytes.  NOT in the other libraries:
// libsliceslice_hip_groups.so holds the fields library's objects plus this file.
//
// A call clears the table and its counters, then runs the hash kernel, the insert kernel, the count kernel, the first-member flags
// per block, the prefix over the blocks and - where a result array asks for it - the emit pass and the group numbers
// (groups_kernels.hpp).  The run form is ss_find_all_runs_device through its public entry point - its count, then both arrays into
// the call's own scratch - and the grouping of those ranges; the line form does the same with the field scan, which leaves one
// record per line.
#include "groups_kernels.hpp"

#include "ss_internal.hpp"

#include "../../include/sliceslice_hip_groups.h"
#include "groups_host.hpp"
#include "matches_launch.hpp"
#include "matches_scratch.hpp"

namespace ss {

hipError_t launch_groups_hash(const GroupsArgs &a, bool fold, hipStream_t st)
{
    const dim3 grid((unsigned)((a.n + kGroupsThreads - 1) / kGroupsThreads)), block(kGroupsThreads);
    if (fold) hipLaunchKernelGGL((groups_hash_kernel<true>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((groups_hash_kernel<false>), grid, block, 0, st, a);
    return hipGetLastError();
}

hipError_t launch_groups_insert(const GroupsArgs &a, bool fold, hipStream_t st)
{
    const dim3 grid((unsigned)((a.n + kGroupsThreads - 1) / kGroupsThreads)), block(kGroupsThreads);
    if (fold) hipLaunchKernelGGL((groups_insert_kernel<true>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((groups_insert_kernel<false>), grid, block, 0, st, a);
    return hipGetLastError();
}

hipError_t launch_groups_count(const GroupsArgs &a, hipStream_t st)
{
    hipLaunchKernelGGL(groups_count_kernel, dim3((unsigned)a.blocks), dim3(kGroupsThreads), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_groups_number(const GroupsArgs &a, hipStream_t st)
{
    hipLaunchKernelGGL(groups_number_kernel, dim3((unsigned)((a.n + kGroupsThreads - 1) / kGroupsThreads)), dim3(kGroupsThreads), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_groups_rank(const GroupsArgs &a, int mode, hipStream_t st)
{
    const dim3 grid((unsigned)a.blocks), block(kGroupsThreads);
    if (mode == kGroupsFlag) hipLaunchKernelGGL((groups_rank_kernel<kGroupsFlag>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((groups_rank_kernel<kGroupsEmit>), grid, block, 0, st, a);
    return hipGetLastError();
}

}  // namespace ss

namespace ssh {
namespace {

static_assert(groups::kMaxRanges == SS_GROUPS_MAX_RANGES && groups::kBlockRanges == SS_GROUPS_BLOCK && ss::kGroupsBlock == SS_GROUPS_BLOCK &&
                  ss::kGroupsLaneMax == SS_GROUPS_LANE_MAX && ss::kGroupsLdsSlots * 12 == SS_GROUPS_LDS_BYTES && groups::kNocase == SS_GROUPS_NOCASE && groups::kWeakHash == SS_GROUPS_WEAK_HASH,
              "groups_host.hpp and groups_launch.hpp restate the header's constants");

// what all three calls refuse about the view, the flags and the stream
int check_groups_view(const char *name, const void *d_haystack, size_t len, unsigned flags, hipStream_t st)
{
    if (len && !d_haystack) return fail(SS_ERR_ARGUMENT, "%s: haystack is NULL", name);
    if (const char *why = groups::check_groups_flags(flags)) return fail(SS_ERR_ARGUMENT, "%s: flags = 0x%x: %s", name, flags, why);
    if (stream_is_capturing(st)) return fail(SS_ERR_ARGUMENT, "%s waits for its stream and cannot be captured into a hipGraph", name);
    return SS_OK;
}

int check_groups_count(const char *name, uint64_t n)
{
    if (n > SS_GROUPS_MAX_RANGES)
        return fail(SS_ERR_ARGUMENT, "%s: %llu ranges; a call takes at most SS_GROUPS_MAX_RANGES = %llu (2^32 - 2)", name, (unsigned long long)n,
                    (unsigned long long)SS_GROUPS_MAX_RANGES);
    return SS_OK;
}

// The grouping of n != 0 ranges behind the argument checks, in scratch[0, groups_scratch_bytes(n)).  The result pointers of `a` are
// set by the caller.
int group_ranges(const char *name, ss::GroupsArgs a, unsigned flags, hipStream_t st, uint8_t *scratch, uint64_t *groups_out)
{
    const uint64_t n = a.n, slots = groups::groups_table_size(n);
    a.weak = (flags & SS_GROUPS_WEAK_HASH) ? 1u : 0u;
    a.tmask = slots - 1;
    a.blocks = groups::groups_blocks(n);
    a.totals = reinterpret_cast<uint64_t *>(scratch);
    a.hash = a.totals + 4;
    a.rank = a.hash + n;
    a.table = reinterpret_cast<uint32_t *>(a.rank + a.blocks);
    a.counter = a.table + slots;
    a.slot = a.counter + slots;
    a.bcount = a.slot + n;
    const bool fold = (flags & SS_GROUPS_NOCASE) != 0;
    HIP_TRY(hipMemsetAsync(a.totals, 0, 32, st));
    HIP_TRY(hipMemsetAsync(a.table, 0xff, slots * sizeof(uint32_t), st));
    HIP_TRY(hipMemsetAsync(a.counter, 0, slots * sizeof(uint32_t), st));
    HIP_TRY(ss::launch_groups_hash(a, fold, st));
    HIP_TRY(ss::launch_groups_insert(a, fold, st));
    HIP_TRY(ss::launch_groups_count(a, st));
    HIP_TRY(ss::launch_groups_rank(a, ss::kGroupsFlag, st));
    HIP_TRY(ss::launch_prefix(a.bcount, a.blocks, a.rank, a.totals, st));
    const bool records = a.capacity != 0 && (a.first || a.count || a.out_b || a.out_e || a.out_n);
    if (!records) a.capacity = 0;
    if (records || a.group) HIP_TRY(ss::launch_groups_rank(a, ss::kGroupsEmit, st));
    if (a.group) HIP_TRY(ss::launch_groups_number(a, st));
    uint64_t totals[2] = {0, 0};
    HIP_TRY(hipMemcpyAsync(totals, a.totals, sizeof(totals), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (totals[1] != 0)
        return fail(SS_ERR_HIP, "%s: %llu ranges found no slot in a table of %llu: the ranges changed under the call", name,
                    (unsigned long long)totals[1], (unsigned long long)slots);
    *groups_out = totals[0];
    return SS_OK;
}

}  // namespace
}  // namespace ssh

using namespace ssh;

extern "C" {

int ss_groups_scratch_bytes(uint64_t n, uint64_t *bytes)
{
    const char *name = "ss_groups_scratch_bytes";
    if (!bytes) return fail(SS_ERR_ARGUMENT, "%s: bytes is NULL", name);
    if (int rc = check_groups_count(name, n)) return rc;
    *bytes = groups::groups_scratch_bytes(n);
    return SS_OK;
}

int ss_group_ranges_device(const void *d_haystack, size_t len, const uint64_t *d_begin, const uint64_t *d_end, uint64_t n, unsigned flags,
                           void *hip_stream, uint64_t *d_first, uint64_t *d_count, uint64_t capacity, uint64_t *d_group, uint64_t *groups_out)
{
    const char *name = "ss_group_ranges_device";
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    if (!groups_out) return fail(SS_ERR_ARGUMENT, "%s: groups is NULL", name);
    if (n != 0 && (!d_begin || !d_end)) return fail(SS_ERR_ARGUMENT, "%s: d_begin or d_end is NULL and n is %llu", name, (unsigned long long)n);
    if (int rc = check_groups_count(name, n)) return rc;
    if (int rc = check_groups_view(name, d_haystack, len, flags, st)) return rc;
    if (n == 0) {
        *groups_out = 0;
        return SS_OK;
    }
    int dev = -1;
    HIP_TRY(hipGetDevice(&dev));
    ScratchLease lease;
    if (int rc = take_scratch(dev, groups::groups_scratch_bytes(n), &lease.sc, st)) return rc;
    ss::GroupsArgs a = {};
    a.hay = static_cast<const uint8_t *>(d_haystack);
    a.len = len;
    a.begin = d_begin;
    a.end = d_end;
    a.n = n;
    a.first = d_first;
    a.count = d_count;
    a.group = d_group;
    a.capacity = capacity;
    uint64_t total = 0;
    if (int rc = group_ranges(name, a, flags, st, lease.sc.d, &total)) return rc;
    lease.done = true;
    *groups_out = total;
    return SS_OK;
}

int ss_group_runs_device(const ss_runs *runs, const void *d_haystack, size_t len, unsigned flags, void *hip_stream, uint64_t *d_begin,
                         uint64_t *d_end, uint64_t *d_count, uint64_t capacity, uint64_t *groups_out, uint64_t *tokens)
{
    const char *name = "ss_group_runs_device";
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    if (!groups_out || !tokens) return fail(SS_ERR_ARGUMENT, "%s: groups or tokens is NULL", name);
    if (!runs) return fail(SS_ERR_ARGUMENT, "%s: runs is NULL", name);
    if (int rc = check_groups_view(name, d_haystack, len, flags, st)) return rc;
    uint64_t n = 0;
    if (int rc = ss_find_all_runs_device(runs, d_haystack, len, hip_stream, nullptr, nullptr, 0, &n)) return rc;    // (the handle's device)
    if (int rc = check_groups_count(name, n)) return rc;
    if (n == 0) {
        *groups_out = 0;
        *tokens = 0;
        return SS_OK;
    }
    int dev = -1;
    HIP_TRY(hipGetDevice(&dev));
    ScratchLease lease;
    const uint64_t own = (groups::groups_scratch_bytes(n) + 7) & ~7ull;
    if (int rc = take_scratch(dev, own + 16 * n, &lease.sc, st)) return rc;
    uint64_t *begin = reinterpret_cast<uint64_t *>(lease.sc.d + own), *end = begin + n, again = 0;
    if (int rc = ss_find_all_runs_device(runs, d_haystack, len, hip_stream, begin, end, n, &again)) return rc;
    lease.done = again != n;                                                    // (both scans have waited: nothing uses the buffer)
    if (again != n)
        return fail(SS_ERR_ARGUMENT, "%s: the haystack changed under the call (%llu runs, then %llu)", name, (unsigned long long)n,
                    (unsigned long long)again);
    ss::GroupsArgs a = {};
    a.hay = static_cast<const uint8_t *>(d_haystack);
    a.len = len;
    a.begin = begin;
    a.end = end;
    a.n = n;
    a.out_b = d_begin;
    a.out_e = d_end;
    a.count = d_count;
    a.capacity = capacity;
    uint64_t total = 0;
    if (int rc = group_ranges(name, a, flags, st, lease.sc.d, &total)) return rc;
    lease.done = true;
    *groups_out = total;
    *tokens = n;
    return SS_OK;
}

int ss_group_lines_device(const void *d_haystack, size_t len, int delimiter, unsigned flags, void *hip_stream, uint64_t *d_begin, uint64_t *d_end,
                          uint64_t *d_number, uint64_t *d_count, uint64_t capacity, uint64_t *groups_out, uint64_t *lines)
{
    const char *name = "ss_group_lines_device";
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    if (!groups_out || !lines) return fail(SS_ERR_ARGUMENT, "%s: groups or lines is NULL", name);
    if (delimiter < 0 || delimiter > 255) return fail(SS_ERR_ARGUMENT, "%s: delimiter %d is not a byte (0 .. 255)", name, delimiter);
    if (int rc = check_groups_view(name, d_haystack, len, flags, st)) return rc;
    // one record per line that spans the whole line: EACH mode, fields 1 .. the last, KEEP_SHORT; the separator is any byte but
    // the delimiter and plays no part
    const unsigned sep = delimiter == 0 ? 1u : 0u;
    uint64_t set[4] = {0, 0, 0, 0};
    set[sep >> 6] |= 1ull << (sep & 63);
    ss_fields *sel = nullptr;
    if (int rc = ss_fields_new(set, SS_FIELDS_EACH, 1, 0, SS_FIELDS_KEEP_SHORT, &sel)) return rc;
    struct Free {
        ss_fields *p;
        ~Free() { ss_fields_free(p); }
    } guard = {sel};
    uint64_t n = 0;
    if (int rc = ss_find_fields_device(sel, d_haystack, len, delimiter, hip_stream, nullptr, nullptr, nullptr, 0, &n)) return rc;
    if (int rc = check_groups_count(name, n)) return rc;
    if (n == 0) {
        *groups_out = 0;
        *lines = 0;
        return SS_OK;
    }
    int dev = -1;
    HIP_TRY(hipGetDevice(&dev));
    ScratchLease lease;
    const uint64_t own = (groups::groups_scratch_bytes(n) + 7) & ~7ull;
    if (int rc = take_scratch(dev, own + 16 * n, &lease.sc, st)) return rc;
    uint64_t *begin = reinterpret_cast<uint64_t *>(lease.sc.d + own), *end = begin + n, again = 0;
    if (int rc = ss_find_fields_device(sel, d_haystack, len, delimiter, hip_stream, begin, end, nullptr, n, &again)) return rc;
    lease.done = again != n;                                                    // (both scans have waited: nothing uses the buffer)
    if (again != n)
        return fail(SS_ERR_ARGUMENT, "%s: the haystack changed under the call (%llu lines, then %llu)", name, (unsigned long long)n,
                    (unsigned long long)again);
    ss::GroupsArgs a = {};
    a.hay = static_cast<const uint8_t *>(d_haystack);
    a.len = len;
    a.begin = begin;
    a.end = end;
    a.n = n;
    a.out_b = d_begin;
    a.out_e = d_end;
    a.out_n = d_number;                                                         // (record k is line k + 1)
    a.count = d_count;
    a.capacity = capacity;
    uint64_t total = 0;
    if (int rc = group_ranges(name, a, flags, st, lease.sc.d, &total)) return rc;
    lease.done = true;
    *groups_out = total;
    *lines = n;
    return SS_OK;
}

}  // extern "C"
