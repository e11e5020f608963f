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
#include "matches_batched_launch.hpp"
#include "matches_scratch.hpp"

namespace ssh {
namespace {

// As ss_batched.hip: workgroups aimed at per CU in total, and the shortest slice worth a workgroup (16 KiB tiles).
constexpr unsigned kAllWgsPerCu = 96;
constexpr uint32_t kAllMinTiles = 2;

struct BatchedAllCall {
    int dev = 0;
    uint32_t slices = 1;
    ss::BatchedAllRanges ranges;
};

int prepare(BatchedAllCall *c, const char *who, const void *d_haystacks, const uint64_t *d_hay_begin, const uint64_t *d_hay_end,
            const void *d_needles, const uint64_t *d_needle_begin, const uint64_t *d_needle_end, size_t count, hipStream_t st)
{
    if (!d_hay_begin || !d_hay_end || !d_needle_begin || !d_needle_end) return fail(SS_ERR_ARGUMENT, "NULL argument");
    HIP_TRY(hipGetDevice(&c->dev));
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(st, &cap) == hipSuccess && cap != hipStreamCaptureStatusNone)
        return fail(SS_ERR_ARGUMENT, "%s keeps scratch that later calls take over and cannot be captured into a hipGraph", who);
    (void)hipGetLastError();
    DeviceInfo di;
    if (int rc = device_info(c->dev, &di)) return rc;
    if (count > 0x3fffffffull) return fail(SS_ERR_ARGUMENT, "too many problems");
    // count x slices < 96 x CUs + count: within gridDim.x for every count that got here
    const uint64_t slices = ((uint64_t)di.cus * kAllWgsPerCu + count - 1) / count;
    if ((uint64_t)count * slices > 0x7fffffffull) return fail(SS_ERR_ARGUMENT, "too many problems for a device of %d compute units", di.cus);
    c->slices = (uint32_t)slices;
    c->ranges = {d_haystacks, d_hay_begin, d_hay_end, d_needles, d_needle_begin, d_needle_end};
    return SS_OK;
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
    HIP_TRY(ss::launch_batched_all_plan(c.ranges, count, descs, colds, c.slices, kAllMinTiles, d_counts, st));
    const ss::BatchedAllScan scan = {descs, colds, d_needles, d_counts, nullptr, nullptr, nullptr, 0, ss::kBatchedAllCount};
    HIP_TRY(ss::launch_batched_all_scan(scan, count, c.slices, lds_pad(), st));
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
    const uint64_t blocks = (uint64_t)count * c.slices;
    // [descriptors][cold parts][total u64][rank u64 x blocks][count u64 x blocks]
    const size_t plan_bytes = count * (ss::kBatchedAllDescBytes + ss::kBatchedAllColdBytes);
    ScratchLease lease;
    if (int rc = take_scratch(c.dev, plan_bytes + 8 + blocks * 16, &lease.sc, st)) return rc;
    uint8_t *descs = lease.sc.d, *colds = descs + count * ss::kBatchedAllDescBytes;
    uint64_t *d_total = reinterpret_cast<uint64_t *>(lease.sc.d + plan_bytes);
    uint64_t *d_rank = d_total + 1, *d_wg = d_rank + blocks;
    HIP_TRY(ss::launch_batched_all_plan(c.ranges, count, descs, colds, c.slices, kAllMinTiles, nullptr, st));
    const ss::BatchedAllScan counting = {descs, colds, d_needles, nullptr, d_wg, nullptr, nullptr, 0, ss::kBatchedAllCountPerWorkgroup};
    HIP_TRY(ss::launch_batched_all_scan(counting, count, c.slices, lds_pad(), st));
    HIP_TRY(ss::launch_prefix64(d_wg, blocks, d_rank, d_total, st));
    HIP_TRY(ss::launch_batched_rows(d_rank, d_total, count, c.slices, d_row_begin, d_counts, st));
    if (capacity) {
        const ss::BatchedAllScan emitting = {descs, colds, d_needles, nullptr, d_wg, d_rank, d_offsets, capacity, ss::kBatchedAllEmit};
        HIP_TRY(ss::launch_batched_all_scan(emitting, count, c.slices, lds_pad(), st));
    }
    HIP_TRY(hipMemcpyAsync(lease.sc.h, d_total, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    lease.done = true;
    *total = *lease.sc.h;
    return SS_OK;
}

}  // extern "C"
