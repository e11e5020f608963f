// needleset_launch.hpp - argument block and host-side entry point of the needle-set kernels (needleset_kernels.hpp; defined and
// used in ss_needleset.hip).
#pragma once
#include "lines_launch.hpp"
#include "needleset_tables.hpp"

namespace ss {

constexpr int kSetSum = 0, kSetEmit = 1, kSetEmitInv = 2;
constexpr int kSetU = 4;                                        // pieces of 1 KiB per wave and tile
constexpr int kSetTiles = 8;                                    // tiles per workgroup
constexpr uint64_t kSetTileChunks = (uint64_t)kWavesPerBlock * kSetU * 64;      // 16-byte chunks of a tile
constexpr uint64_t kSetPartBytes = kSetTileChunks * 16 * kSetTiles;             // bytes of the view per workgroup

struct SetArgs {
    const uint8_t *base;        // the 16-byte aligned address at or below the view
    const uint8_t *hay;         // the view's first byte: base + mis
    uint64_t mis, len;
    uint64_t nchunks;           // chunks from `base` that hold a byte of the view
    uint64_t ntiles;
    SetView tv;                 // the set's tables in device memory
    LineSum *sum;               // kSetSum: written; kSetEmitInv: read
    const LinePre *pre;         // emit: the state in front of every workgroup
    uint64_t *begin, *end, *number;
    uint64_t capacity;
    uint32_t delim, how;        // how: SS_BOUND_WORD | SS_BOUND_LINE
};

// ceil(ntiles / kSetTiles) workgroups of kBlock lanes
hipError_t launch_set_scan(const SetArgs &sa, int mode, hipStream_t st);

}  // namespace ss
