// context_launch.hpp - host-side entry points of the context kernels (context_kernels.hpp; defined in ss_context.hip, the only
// translation unit that holds them: libsliceslice_hip_context.so).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "../../include/sliceslice_hip_context.h"

namespace ss {

// One call's arguments, the same struct for every kernel.  The view is bytes [lo, hi) of the STREAM that starts at `base`, the
// 16-byte aligned address at or below the haystack pointer (lo < 16): the parts are cut at multiples of SS_CONTEXT_PART_BYTES of
// the stream, so that every part is whole aligned chunks.
struct CtxArgs {
    const uint8_t *base;
    uint64_t lo, hi;
    uint64_t parts;
    uint32_t delim;
    uint64_t *cnt;              // [parts] delimiters of the view in the part
    uint64_t *pre;              // [parts] ... in front of it
    uint64_t *ndelim;           // ... in the whole view
    const uint64_t *numbers;    // the caller's line numbers
    uint64_t count;
    uint64_t before, after;
    uint64_t *first;            // [count] output slots the entries in front of it IN ITS BLOCK of kBlock entries own
    uint64_t *bsum, *bpre;      // [blocks] slots the block owns / the blocks in front of it own
    uint64_t *total;            // the size of the output
    uint64_t *out_begin, *out_end, *out_number;
    uint8_t *out_kind;
    uint64_t capacity;
};

hipError_t launch_context_census(const CtxArgs &ca, hipStream_t st);        // cnt
hipError_t launch_context_part_prefix(const CtxArgs &ca, hipStream_t st);   // cnt -> pre, ndelim
hipError_t launch_context_ranges(const CtxArgs &ca, hipStream_t st);        // first, bsum
hipError_t launch_context_block_prefix(const CtxArgs &ca, hipStream_t st);  // bsum -> bpre, total
hipError_t launch_context_fill(const CtxArgs &ca, int cus, hipStream_t st); // out_number, out_kind below the capacity
hipError_t launch_context_select(const CtxArgs &ca, hipStream_t st);        // out_begin, out_end below the capacity

}  // namespace ss
