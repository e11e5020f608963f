// anyof_launch.hpp - host-side entry points of the union kernels (anyof_kernels.hpp; defined in ss_anyof.hip, the only translation
// unit that holds them: libsliceslice_hip_anyof.so).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "../../include/sliceslice_hip_anyof.h"

namespace ss {

// One call's arguments, the same struct for every kernel.  List k is numbers[off[k], off[k + 1]).
struct AnyArgs {
    const uint64_t *numbers;    // the caller's line numbers, every list ascending
    const uint64_t *off;        // [lists + 1] in device memory
    uint32_t lists;
    int complement;
    uint64_t limit;
    uint64_t segs;              // segments of SS_ANYOF_SEGMENT_LINES numbers that 1 .. limit need
    uint64_t *cnt;              // [segs] output numbers of the segment
    uint64_t *pre;              // [segs] ... of the segments in front of it
    uint64_t *total;            // the size of the output
    uint64_t *out;
    uint64_t capacity;
};

hipError_t launch_anyof_count(const AnyArgs &aa, hipStream_t st);       // cnt
hipError_t launch_anyof_prefix(const AnyArgs &aa, hipStream_t st);      // cnt -> pre, total
hipError_t launch_anyof_emit(const AnyArgs &aa, hipStream_t st);        // out below the capacity

}  // namespace ss
