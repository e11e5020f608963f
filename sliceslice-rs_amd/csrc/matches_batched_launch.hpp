// matches_batched_launch.hpp - host-side entry points of the batched all-matches kernels (defined in scan_inst_all_batched.hip,
// used by ss_matches_batched.hip).  The descriptors and cold records stay inside the kernels' translation unit: the host sees bytes.
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>

namespace ss {

struct BatchArgs;               // batched_types.hpp: the batch as the caller names it (ssh::fill_batch_args)
constexpr size_t kBatchedAllDescBytes = 64, kBatchedAllColdBytes = 64;     // per problem: BatchDesc, BatchCold
constexpr uint32_t kBatchedAllCount = 0, kBatchedAllCountPerWorkgroup = 1, kBatchedAllEmit = 2;

// Descriptors and cold parts of `count` problems for a scan grid of `nslices` workgroups per problem (slices no shorter than
// `min_tiles` tiles); `counts` (may be null) takes every problem's initial count: 0, or len + 1 for the empty needle.
hipError_t launch_batched_all_plan(const BatchArgs &a, uint64_t count, void *descs, void *colds, uint32_t nslices, uint32_t min_tiles,
                                   uint64_t *counts, hipStream_t st);
struct BatchedAllScan {
    const void *descs, *colds;
    const void *needles;
    uint64_t *counts;           // kBatchedAllCount
    uint64_t *wg_count;         // kBatchedAllCountPerWorkgroup (written), kBatchedAllEmit (read): count * nslices words
    const uint64_t *wg_rank;    // kBatchedAllEmit
    uint64_t *out;
    uint64_t capacity;
    uint32_t mode;
};
// count * nslices workgroups (at most 2^31 - 1), problem-major; lds_pad: unused dynamic LDS that sets the workgroups per CU
hipError_t launch_batched_all_scan(const BatchedAllScan &s, uint64_t count, uint32_t nslices, uint32_t lds_pad, hipStream_t st);
// rank[k] = count[0] + ... + count[k-1] for k < n, *total = the sum of all n (64-bit counts; launch_prefix takes 32-bit ones)
hipError_t launch_prefix64(const uint64_t *count, uint64_t n, uint64_t *rank, uint64_t *total, hipStream_t st);
// row_begin[p] = wg_rank[p * nslices] for p < count, row_begin[count] = *total; counts (may be null) = the rows' lengths
hipError_t launch_batched_rows(const uint64_t *wg_rank, const uint64_t *total, uint64_t count, uint32_t nslices, uint64_t *row_begin,
                               uint64_t *counts, hipStream_t st);

}  // namespace ss
