// matches_launch.hpp - host-side entry points of the all-matches kernels (defined in scan_inst_all.hip, used by ss_matches.hip).
#pragma once
#include "scan_launch.hpp"

namespace ss {

// The all-matches scan of one Problem: mode 0 / 2 / 3 (3 runs the MODE 2 kernel), U = 4, non-temporal loads; sh.tpb >= 1
// (contiguous tiles per workgroup).  Returns false when no kernel fits (nothing has been launched then); scan_choice.hpp chooses.
// `bound` is the mode word of the scans that look at an occurrence's neighbour bytes (bounded_launch.hpp); every other scan takes 0
// and ignores it.
bool launch_scan_all(const Problem &pr, int q, int mode, bool one_byte, const Shape &sh, hipStream_t st, const AllArgs &aa, uint32_t bound);
// (the host side takes the scan as a value of this type: ss_matches.hip, matches_host.hpp)
typedef bool (*ScanAllFn)(const Problem &pr, int q, int mode, bool one_byte, const Shape &sh, hipStream_t st, const AllArgs &aa, uint32_t bound);
// rank[k] = count[0] + ... + count[k-1] for k < n, *total = the sum of all n
hipError_t launch_prefix(const uint32_t *count, uint64_t n, uint64_t *rank, uint64_t *total, hipStream_t st);
// out[i] = i for i < count
hipError_t launch_iota(uint64_t *out, uint64_t count, hipStream_t st);
hipError_t launch_store_u64(uint64_t *out, uint64_t v, hipStream_t st);

}  // namespace ss
