// scan_inst_all.hip - the all-matches kernels (scan_all_kernel, scan_kernels.hpp) and their small helpers: one scan kernel per
// (Q, MODE, one-byte) combination that find() has - 4 Q x MODE 0, 4 Q x MODE 2, one-byte: 9, chosen by scan_choice.hpp - plus the
// prefix sum of the workgroup counts (prefix_kernel.hpp) and the empty needle's fill.  Compiled into libsliceslice_hip_matches.so
// only (ss_matches.hip is the host side).
#include "scan_choice.hpp"
#include "matches_launch.hpp"
#include "prefix_kernel.hpp"

namespace ss {

namespace {

// The empty needle: offsets 0 .. count - 1
__global__ void iota_kernel(uint64_t *out, uint64_t count)
{
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += (uint64_t)gridDim.x * blockDim.x) out[i] = i;
}

__global__ void store_u64_kernel(uint64_t *out, uint64_t v) { *out = v; }

}  // namespace

bool launch_scan_all(const Problem &pr, int q, int mode, bool one_byte, const Shape &sh, hipStream_t st, const AllArgs &aa, uint32_t)
{
    return choose_scan_kernel(q, mode, one_byte, [&](auto Q, auto MODE, auto ONE_BYTE) {
        scan_all_kernel<decltype(Q)::value, decltype(MODE)::value, decltype(ONE_BYTE)::value>
            <<<dim3(sh.blocks), dim3(sh.block), scan_dyn_lds(sh), st>>>(pr, aa, sh.tpb);
    });
}

hipError_t launch_prefix(const uint32_t *count, uint64_t n, uint64_t *rank, uint64_t *total, hipStream_t st)
{
    prefix_kernel<uint32_t><<<1, kPrefixThreads, 0, st>>>(count, n, rank, total);
    return hipGetLastError();
}

hipError_t launch_iota(uint64_t *out, uint64_t count, hipStream_t st)
{
    if (count == 0) return hipSuccess;
    uint64_t blocks = (count + kBlock - 1) / kBlock;
    if (blocks > 4096) blocks = 4096;
    iota_kernel<<<(unsigned)blocks, kBlock, 0, st>>>(out, count);
    return hipGetLastError();
}

hipError_t launch_store_u64(uint64_t *out, uint64_t v, hipStream_t st)
{
    store_u64_kernel<<<1, 1, 0, st>>>(out, v);
    return hipGetLastError();
}

}  // namespace ss
