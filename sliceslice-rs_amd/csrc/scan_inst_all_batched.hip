// scan_inst_all_batched.hip - the batched all-matches kernels (batched_all_kernels.hpp) and their launches: the plan kernel (and
// ss_batched.hip's cold kernel) in front of the scan, scan_all_batched_kernel, the 64-bit prefix sum and the rows.  Compiled into
// libsliceslice_hip_matches_batched.so only (ss_matches_batched.hip is the host side).
#include "batched_all_kernels.hpp"
#include "matches_batched_launch.hpp"
#include "prefix_kernel.hpp"

namespace ss {

static_assert(sizeof(BatchDesc) == kBatchedAllDescBytes && sizeof(BatchCold) == kBatchedAllColdBytes, "the host sizes its scratch by these");

hipError_t launch_batched_all_plan(const BatchArgs &a, uint64_t count, void *descs, void *colds, uint32_t nslices, uint32_t min_tiles,
                                   uint64_t *counts, hipStream_t st)
{
    const unsigned blocks = (unsigned)((count + kBlock - 1) / kBlock);
    batch_all_plan_kernel<<<dim3(blocks), dim3(kBlock), 0, st>>>(a, count, static_cast<BatchDesc *>(descs), nslices, min_tiles, counts);
    if (hipError_t e = hipGetLastError()) return e;
    // (static classes, bool-style idle state words: nobody reads them)
    return launch_batch_cold(a, static_cast<const BatchDesc *>(descs), count, static_cast<BatchCold *>(colds), nullptr, 0, st);
}

hipError_t launch_batched_all_scan(const BatchedAllScan &s, uint64_t count, uint32_t nslices, uint32_t lds_pad, hipStream_t st)
{
    const uint64_t blocks = count * nslices;
    if (blocks == 0 || blocks > 0x7fffffffull) return hipErrorInvalidValue;
    const BatchedAllArgs aa = {static_cast<const BatchDesc *>(s.descs), static_cast<const BatchCold *>(s.colds),
                               static_cast<const uint8_t *>(s.needles), s.counts, s.wg_count, s.wg_rank, s.out, s.capacity, nslices, s.mode};
    if (s.mode == kBatchedAllEmit) scan_all_batched_kernel<true><<<dim3((unsigned)blocks), dim3(kBlock), lds_pad, st>>>(aa);
    else scan_all_batched_kernel<false><<<dim3((unsigned)blocks), dim3(kBlock), lds_pad, st>>>(aa);
    return hipGetLastError();
}

hipError_t launch_prefix64(const uint64_t *count, uint64_t n, uint64_t *rank, uint64_t *total, hipStream_t st)
{
    prefix_kernel<uint64_t><<<1, kPrefixThreads, 0, st>>>(count, n, rank, total);
    return hipGetLastError();
}

hipError_t launch_batched_rows(const uint64_t *wg_rank, const uint64_t *total, uint64_t count, uint32_t nslices, uint64_t *row_begin,
                               uint64_t *counts, hipStream_t st)
{
    const unsigned blocks = (unsigned)((count + 1 + kBlock - 1) / kBlock);
    batch_rows_kernel<<<dim3(blocks), dim3(kBlock), 0, st>>>(wg_rank, total, count, nslices, row_begin, counts);
    return hipGetLastError();
}

}  // namespace ss
