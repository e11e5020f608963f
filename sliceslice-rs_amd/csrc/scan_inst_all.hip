// scan_inst_all.hip - the all-matches kernels (scan_all_kernel, scan_kernels.hpp) and their small helpers: one scan kernel per
// (Q, MODE, one-byte) combination that find() has - 4 Q x MODE 0, 4 Q x MODE 2, one-byte: 9 - plus the prefix sum of the
// workgroup counts (prefix_kernel.hpp) and the empty needle's fill.  Compiled into libsliceslice_hip_matches.so only (ss_matches.hip is the host side).
#include "scan_launch.hpp"
#include "matches_launch.hpp"
#include "prefix_kernel.hpp"

namespace ss {

namespace {

template <int Q, int MODE, bool ONE_BYTE>
void launch_all_one(const Problem &pr, const Shape &sh, hipStream_t st, const AllArgs &aa)
{
    const uint32_t dyn_lds = sh.lds_pad + (sh.block / kWave) * kNeedleLds;   // one needle slice per wave
    scan_all_kernel<Q, MODE, ONE_BYTE><<<dim3(sh.blocks), dim3(sh.block), dyn_lds, st>>>(pr, aa, sh.tpb);
}

// The empty needle: offsets 0 .. count - 1
__global__ void iota_kernel(uint64_t *out, uint64_t count)
{
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += (uint64_t)gridDim.x * blockDim.x) out[i] = i;
}

__global__ void store_u64_kernel(uint64_t *out, uint64_t v) { *out = v; }

}  // namespace

bool launch_scan_all(const Problem &pr, int q, int mode, bool one_byte, const Shape &sh, hipStream_t st, const AllArgs &aa)
{
    if (one_byte) return launch_all_one<0, 0, true>(pr, sh, st, aa), true;
    if (mode == 3) mode = 2;                  // a pair-alone searcher: the MODE 2 kernel with its third byte, as find() does
#define SS_CASE(QQ, MM)                                                                            \
    case (QQ) * 4 + (MM):                                                                          \
        return launch_all_one<QQ, MM, false>(pr, sh, st, aa), true;
    switch (q * 4 + mode) {
        SS_CASE(0, 0) SS_CASE(0, 2) SS_CASE(1, 0) SS_CASE(1, 2)
        SS_CASE(2, 0) SS_CASE(2, 2) SS_CASE(3, 0) SS_CASE(3, 2)
    }
#undef SS_CASE
    return false;
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
