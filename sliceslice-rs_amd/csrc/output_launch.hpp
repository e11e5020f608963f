// output_launch.hpp - argument block and host-side entry points of the output kernels (output_kernels.hpp; defined and used in
// ss_output.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "../../include/sliceslice_hip_output.h"

namespace ss {

constexpr int kOutputThreads = 1024;                            // lanes per workgroup of the size and the start kernel
constexpr int kOutputCopyThreads = 256;                         // ... of the copy kernel
constexpr uint32_t kOutputRun = 512;                            // records a copy workgroup stages in LDS at a time

struct OutputArgs {
    const uint8_t *hay;         // the view (any alignment; may be NULL with len == 0)
    uint64_t len;
    const uint64_t *begin, *end;
    const uint64_t *number;     // NULL: no flags
    const uint8_t *kind;        // NULL: every record prints `:`
    uint64_t count;
    uint64_t blocks;            // ceil(count / SS_OUTPUT_BLOCK)
    int terminator;             // -1: none
    unsigned flags;
    // scratch
    uint64_t *sum;              // per block: its bytes
    uint64_t *rank;             // per block: the bytes in front of it
    uint64_t *total;
    // starts
    uint64_t *starts;           // count + 1 entries
    // copy
    uint8_t *out_base;          // the 16-byte aligned address at or below d_out
    uint64_t out_lo, out_hi;    // the output is out_base[out_lo, out_hi)
    uint64_t chunks;            // chunks of SS_OUTPUT_CHUNK from out_base
};

// ceil(count / SS_OUTPUT_BLOCK) workgroups of kOutputThreads lanes; then the prefix over the blocks' bytes (prefix_kernel.hpp)
// -> rank, *total
hipError_t launch_output_sizes(const OutputArgs &a, hipStream_t st);
hipError_t launch_output_starts(const OutputArgs &a, hipStream_t st);
// `chunks` workgroups of kOutputCopyThreads lanes
hipError_t launch_output_copy(const OutputArgs &a, hipStream_t st);

}  // namespace ss
