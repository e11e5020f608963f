// prefix_kernel.hpp - the rank of every workgroup in the output of a find-all call: the exclusive prefix sum of the workgroup
// counts.  Instantiated for 32-bit counts in scan_inst_all.hip (launch_prefix) and for 64-bit ones in scan_inst_all_batched.hip
// (launch_prefix64).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace ss {

// rank[k] = count[0] + ... + count[k-1] for k < n, *total = the sum of all n.  One workgroup: thread t sums a contiguous run of the
// counts, the runs' sums are scanned in LDS, and every thread writes the ranks of its run.  The counts of a 1 GiB haystack are
// 256 KiB.
constexpr int kPrefixThreads = 1024;
template <class CountT>
__global__ void __launch_bounds__(kPrefixThreads) prefix_kernel(const CountT *count, uint64_t n, uint64_t *rank, uint64_t *total)
{
    __shared__ uint64_t s_run[kPrefixThreads];
    const uint64_t per = (n + kPrefixThreads - 1) / kPrefixThreads;
    const uint64_t b0 = (uint64_t)threadIdx.x * per, b = b0 < n ? b0 : n, e = b + per < n ? b + per : n;
    uint64_t sum = 0;
    for (uint64_t k = b; k < e; ++k) sum += count[k];
    s_run[threadIdx.x] = sum;
    __syncthreads();
    for (int k = 1; k < kPrefixThreads; k <<= 1) {           // Hillis-Steele inclusive scan of the run sums
        const uint64_t v = threadIdx.x >= (unsigned)k ? s_run[threadIdx.x - k] : 0ull;
        __syncthreads();
        s_run[threadIdx.x] += v;
        __syncthreads();
    }
    uint64_t r = s_run[threadIdx.x] - sum;
    for (uint64_t k = b; k < e; ++k) {
        rank[k] = r;
        r += count[k];
    }
    if (threadIdx.x == kPrefixThreads - 1) *total = s_run[threadIdx.x];
}

}  // namespace ss
