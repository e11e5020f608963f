// setmatches_launch.hpp - argument block and host-side entry points of the occurrence kernels of a needle set
// (setmatches_kernels.hpp; defined and used in ss_setmatches.hip).
#pragma once
#include "needleset_launch.hpp"

namespace ss {

constexpr int kSetAllCount = 0, kSetAllEmit = 1;

struct SetAllArgs {
    const uint8_t *base;        // the 16-byte aligned address at or below the view
    const uint8_t *hay;         // the view's first byte: base + mis
    uint64_t mis, len;
    uint64_t nchunks;           // chunks from `base` that hold a byte of the view
    uint64_t ntiles;
    SetView tv;                 // the set's tables in device memory
    SetRanks tr;                // ... and its needles' ranks and histogram slots
    uint64_t *counts;           // count: one bin per rank (added to), or NULL
    uint64_t *total;            // count: every workgroup adds its pairs here, or NULL
    uint64_t *wg;               // count: the pairs of every workgroup (written), or NULL; emit: read
    const uint64_t *wg_rank;    // emit: the pairs in front of every workgroup
    uint64_t *offsets;          // emit: either may be NULL
    uint32_t *ranks;
    uint64_t capacity;
    uint32_t how;               // 0 or SS_BOUND_WORD
};

// ceil(ntiles / kSetTiles) workgroups of kBlock lanes
hipError_t launch_set_all(const SetAllArgs &a, int mode, hipStream_t st);
// rank[k] = count[0] + ... + count[k - 1], *total = their sum (prefix_kernel.hpp over 64-bit counts)
hipError_t launch_set_prefix(const uint64_t *count, uint64_t n, uint64_t *rank, uint64_t *total, hipStream_t st);

}  // namespace ss
