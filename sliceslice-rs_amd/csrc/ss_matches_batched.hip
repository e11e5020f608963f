// ss_matches_batched.hip - every occurrence for a batch of problems (include/sliceslice_hip_matches_batched.h): ss_count_batched,
// ss_find_all_batched.  NOT in libsliceslice_hip.so or libsliceslice_hip_matches.so: libsliceslice_hip_matches_batched.so holds the
// matches library's objects plus this file and scan_inst_all_batched.hip.
//
//   count      plan kernel (descriptors; the initial counts, complete for problems without a scan) -> cold kernel -> the scan grid,
//              in which every workgroup with matches adds its count to its problem's 64-bit word.  Three launches, no wait.
//   find_all   plan -> cold -> a count pass that writes one 64-bit count per workgroup -> their exclusive prefix sum (one
//              workgroup) -> rows and counts from the ranks (one lane per problem) -> an emit pass over the same grid in which only
//              the workgroups that hold one of the first `capacity` matches re-read their tiles and write their offsets at their
//              rank.  The grid is problem-major and a slice is a contiguous run of tiles, so workgroup order is (problem, address)
//              order and the rows land sorted.
// The grid is sized from the problem count alone, by the rule of ss_search_batched (batch_shape, ss_batched.hip); ss_find_all_batched
// does not read the plan kernel's view of the lengths back either - the header says what that means for one long problem among many.
// Nothing is remembered between calls but free scratch buffers: static byte classes, no sampling, no census.
#include "ss_internal.hpp"

#include "../../include/sliceslice_hip_matches_batched.h"
#include "batched_types.hpp"
#include "matches_batched_launch.hpp"
#include "matches_scratch.hpp"

namespace ssh {
namespace {

struct BatchedAllCall {
    int dev = 0;
    BatchShape shape = {1, 1};      // the grid rule of ss_search_batched (batch_shape, ss_batched.hip)
    ss::BatchArgs args;
};

int prepare(BatchedAllCall *c, const char *who, const void *d_haystacks, const uint64_t *d_hay_begin, const uint64_t *d_hay_end,
            const void *d_needles, const uint64_t *d_needle_begin, const uint64_t *d_needle_end, size_t count, hipStream_t st)
{
    if (int rc = fill_batch_args(&c->args, d_haystacks, d_hay_begin, d_hay_end, d_needles, d_needle_begin, d_needle_end, nullptr)) return rc;
    HIP_TRY(hipGetDevice(&c->dev));
    if (stream_is_capturing(st))
        return fail(SS_ERR_ARGUMENT, "%s keeps scratch that later calls take over and cannot be captured into a hipGraph", who);
    return batch_shape(c->dev, count, &c->shape);
}

// four workgroups per CU, as the batched search and the single all-matches scan on random bytes
uint32_t lds_pad() { return occupancy_pad(4, ss::kBlock); }

}  // namespace
}  // namespace ssh

using namespace ssh;

extern "C" {

int ss_count_batched(const void *d_haystacks, const uint64_t *d_hay_begin, const uint64_t *d_hay_end,
                     const void *d_needles, const uint64_t *d_needle_begin, const uint64_t *d_needle_end,
                     size_t count, void *hip_stream, uint64_t *d_counts)
{
    if (count == 0) return SS_OK;
    if (!d_counts) return fail(SS_ERR_ARGUMENT, "NULL argument");
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    BatchedAllCall c;
    if (int rc = prepare(&c, "ss_count_batched", d_haystacks, d_hay_begin, d_hay_end, d_needles, d_needle_begin, d_needle_end, count, st))
        return rc;
    // [descriptors][cold parts]
    ScratchLease lease;
    if (int rc = take_scratch(c.dev, count * (ss::kBatchedAllDescBytes + ss::kBatchedAllColdBytes), &lease.sc, st)) return rc;
    uint8_t *descs = lease.sc.d, *colds = descs + count * ss::kBatchedAllDescBytes;
    HIP_TRY(ss::launch_batched_all_plan(c.args, count, descs, colds, c.shape.slices, c.shape.min_tiles, d_counts, st));
    const ss::BatchedAllScan scan = {descs, colds, d_needles, d_counts, nullptr, nullptr, nullptr, 0, ss::kBatchedAllCount};
    HIP_TRY(ss::launch_batched_all_scan(scan, count, c.shape.slices, lds_pad(), st));
    return lease.release_on(st);
}

int ss_find_all_batched(const void *d_haystacks, const uint64_t *d_hay_begin, const uint64_t *d_hay_end,
                        const void *d_needles, const uint64_t *d_needle_begin, const uint64_t *d_needle_end,
                        size_t count, void *hip_stream, uint64_t *d_counts, uint64_t *d_row_begin,
                        uint64_t *d_offsets, uint64_t capacity, uint64_t *total)
{
    if (!total || !d_row_begin) return fail(SS_ERR_ARGUMENT, "NULL argument");
    if (capacity && !d_offsets) return fail(SS_ERR_ARGUMENT, "offsets are NULL with a capacity of %llu", (unsigned long long)capacity);
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    if (count == 0) {
        HIP_TRY(hipMemsetAsync(d_row_begin, 0, sizeof(uint64_t), st));
        HIP_TRY(hipStreamSynchronize(st));
        *total = 0;
        return SS_OK;
    }
    BatchedAllCall c;
    if (int rc = prepare(&c, "ss_find_all_batched", d_haystacks, d_hay_begin, d_hay_end, d_needles, d_needle_begin, d_needle_end, count, st))
        return rc;
    const uint64_t blocks = (uint64_t)count * c.shape.slices;
    // [descriptors][cold parts][total u64][rank u64 x blocks][count u64 x blocks]
    const size_t plan_bytes = count * (ss::kBatchedAllDescBytes + ss::kBatchedAllColdBytes);
    ScratchLease lease;
    if (int rc = take_scratch(c.dev, plan_bytes + 8 + blocks * 16, &lease.sc, st)) return rc;
    uint8_t *descs = lease.sc.d, *colds = descs + count * ss::kBatchedAllDescBytes;
    uint64_t *d_total = reinterpret_cast<uint64_t *>(lease.sc.d + plan_bytes);
    uint64_t *d_rank = d_total + 1, *d_wg = d_rank + blocks;
    HIP_TRY(ss::launch_batched_all_plan(c.args, count, descs, colds, c.shape.slices, c.shape.min_tiles, nullptr, st));
    const ss::BatchedAllScan counting = {descs, colds, d_needles, nullptr, d_wg, nullptr, nullptr, 0, ss::kBatchedAllCountPerWorkgroup};
    HIP_TRY(ss::launch_batched_all_scan(counting, count, c.shape.slices, lds_pad(), st));
    HIP_TRY(ss::launch_prefix64(d_wg, blocks, d_rank, d_total, st));
    HIP_TRY(ss::launch_batched_rows(d_rank, d_total, count, c.shape.slices, d_row_begin, d_counts, st));
    if (capacity) {
        const ss::BatchedAllScan emitting = {descs, colds, d_needles, nullptr, d_wg, d_rank, d_offsets, capacity, ss::kBatchedAllEmit};
        HIP_TRY(ss::launch_batched_all_scan(emitting, count, c.shape.slices, lds_pad(), st));
    }
    HIP_TRY(hipMemcpyAsync(lease.sc.h, d_total, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    lease.done = true;
    *total = *lease.sc.h;
    return SS_OK;
}

}  // extern "C"
