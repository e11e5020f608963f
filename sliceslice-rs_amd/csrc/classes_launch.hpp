// classes_launch.hpp - argument block and host-side entry points of the byte-class kernels (classes_kernels.hpp; defined and used in
// ss_classes.hip).
#pragma once
#include "masked_launch.hpp"

namespace ss {

constexpr uint32_t kClassesMaxInexact = 1024;                   // SS_CLASSES_MAX_INEXACT: entries of the check list
constexpr uint32_t kClassesMaxDistinct = 64;                    // SS_CLASSES_MAX_DISTINCT: bitmaps of 8 dwords

struct ClassArgs {
    MaskedArgs m;               // the view, the filter and the (value, mask) table of the COVERS; the modes are masked_launch.hpp's
    const uint32_t *ctab;       // device: nbits dwords of bitmaps (8 per distinct inexact set: bit b & 31 of dword b >> 5), then the
                                // check list, nchecks dwords: position | (first bitmap dword of the set) << 16, rarest set first
    uint32_t nbits, nchecks;    // (nchecks == 0: every position is exactly its cover and the exact test is skipped)
};

// ceil(ntiles / kSetTiles) workgroups of kBlock lanes
hipError_t launch_classes_all(const ClassArgs &a, int mode, hipStream_t st);
hipError_t launch_classes_lines(const ClassArgs &a, int mode, hipStream_t st);

}  // namespace ss
