// masked_launch.hpp - argument block and host-side entry points of the masked-pattern kernels (masked_kernels.hpp; defined and used
// in ss_masked.hip).
#pragma once
#include "setmatches_launch.hpp"

namespace ss {

constexpr int kMaskedCount = 0, kMaskedEmit = 1;                // masked_all_kernel
constexpr int kMaskedSum = 0, kMaskedLineEmit = 1;              // masked_lines_kernel
constexpr uint32_t kMaskedMaxLen = 4096;                        // SS_MASKED_MAX_LEN
constexpr uint32_t kMaskedMaxWords = kMaskedMaxLen / 4;

struct MaskedArgs {
    const uint8_t *base;        // the 16-byte aligned address at or below the view
    const uint8_t *hay;         // the view's first byte: base + mis
    uint64_t mis, len;          // (n <= len: the host answers every other call itself)
    uint64_t nchunks;           // chunks from `base` that hold a byte of the view
    uint64_t ntiles;
    const uint32_t *tab;        // device: (value, mask) dword pairs, nw of them; the bytes behind n have value 0 and mask 0
    uint32_t n, nw;             // pattern bytes, ceil(n / 4)
    uint32_t a, d;              // the filter: pattern positions a and a + d (d == 0: one byte)
    uint32_t v0x4, m0x4, v1x4, m1x4;    // their value and mask, splatted (m1x4 == 0 with d == 0)
    // occurrences
    uint64_t *total;            // count: every workgroup adds its occurrences here, or NULL
    uint64_t *wg;               // count: the occurrences of every workgroup (written), or NULL; emit: read
    const uint64_t *wg_rank;    // emit: the occurrences in front of every workgroup
    uint64_t *offsets;          // emit
    uint64_t capacity;          // emit, line emit
    // lines
    LineSum *sum;               // kMaskedSum: written
    const LinePre *pre;         // kMaskedLineEmit: the state in front of every workgroup
    uint64_t *begin, *end, *number;
    uint32_t delim;
    uint32_t accepts;           // some pattern position accepts the delimiter: candidates are also tested against it
};

// ceil(ntiles / kSetTiles) workgroups of kBlock lanes
hipError_t launch_masked_all(const MaskedArgs &a, int mode, hipStream_t st);
hipError_t launch_masked_lines(const MaskedArgs &a, int mode, hipStream_t st);

}  // namespace ss
