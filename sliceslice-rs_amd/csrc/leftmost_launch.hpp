// leftmost_launch.hpp - argument blocks and host-side entry points of the leftmost-longest selection and the set-replace kernels
// (leftmost_kernels.hpp; defined and used in ss_leftmost.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "../../include/sliceslice_hip_leftmost.h"

namespace ss {

constexpr int kLeftmostThreads = 1024;                          // lanes per workgroup of the selection kernels
constexpr int kLeftmostCopyThreads = 256;                       // ... of the copy kernel
constexpr uint32_t kLeftmostNone = 0xffffffffu;                 // head: the block holds no head; entry: no chain enters the block
constexpr int kLeftmostExitBits = 48;                           // a record: selections << 48 | exit
constexpr uint64_t kLeftmostExitMask = (1ull << kLeftmostExitBits) - 1;
constexpr uint32_t kLeftmostBlobPad = 16;                       // bytes behind the replacement blob that a 16-byte load may touch

struct LeftmostArgs {
    const uint64_t *offsets;    // ascending, may repeat (the caller's contract)
    const uint64_t *lengths;    // one per entry, ascending within a run of equal offsets; or NULL, and then ...
    const uint32_t *ranks;      // ... the rank of every entry and
    const uint64_t *rank_len;   // the length of every rank
    uint64_t count;
    uint64_t blocks;            // ceil(count / SS_LEFTMOST_BLOCK)
    // scratch
    uint64_t *rec;              // `count` records: the selections of the walk that enters its block at this entry, and its exit (the
                                // global index of the first entry at or beyond the end of the last selected one); written for the
                                // entries up to the block's first head, for every entry of a block without one
    uint32_t *head;             // per block: the local index of its first head, or kLeftmostNone
    uint32_t *entry;            // per block: the local index at which the chain enters it, or kLeftmostNone (skipped whole)
    uint64_t *cnt;              // per block: its selections (before the chain pass: the largest length of its entries)
    uint64_t *rank;             // per block: the selections in front of it
    uint64_t *total;            // [0] the selections, [1] the largest length of the list
    // emit
    uint64_t *out;              // the selected offsets, or NULL
    uint64_t *which;            // their indices in the list, or NULL
    uint32_t *out_ranks;        // ranks[index], or NULL
    uint64_t capacity;
};

// the length and the replacement of a rank, as the replace kernels see them
struct LeftmostRank {
    uint64_t needle_len, rep_off, rep_len;
};

struct LeftmostReplaceArgs {
    const uint8_t *hay;         // the view (any alignment)
    uint64_t len;
    const uint64_t *sel;        // the selected offsets, ascending
    const uint32_t *sel_rank;   // their ranks
    uint64_t nsel;
    uint64_t blocks;            // ceil(nsel / SS_LEFTMOST_BLOCK)
    const LeftmostRank *table;  // per rank
    const uint8_t *blob;        // the replacements, one behind the other, kLeftmostBlobPad bytes behind the last
    // scratch
    uint64_t *sum;              // per block: the sum of (replacement length - needle length), modulo 2^64
    uint64_t *rank;             // per block: that sum in front of it
    uint64_t *total;
    uint64_t *starts;           // nsel entries: the output offset of every selection's replacement
    // copy
    uint8_t *out_base;          // the 16-byte aligned address at or below d_out
    uint64_t out_lo, out_hi;    // the output is out_base[out_lo, out_hi)
    uint64_t chunks;            // chunks of SS_OUTPUT_CHUNK from out_base
};

// the largest length: ceil(count / SS_LEFTMOST_BLOCK) workgroups, then one
hipError_t launch_leftmost_longest(const LeftmostArgs &a, hipStream_t st);
hipError_t launch_leftmost_block(const LeftmostArgs &a, hipStream_t st);
// one workgroup: every block's entry and selections; then the prefix over the selections (prefix_kernel.hpp) -> rank, total[0]
hipError_t launch_leftmost_chain(const LeftmostArgs &a, hipStream_t st);
hipError_t launch_leftmost_emit(const LeftmostArgs &a, hipStream_t st);
// the blocks' sums and their prefix; the starts; `chunks` workgroups of kLeftmostCopyThreads lanes
hipError_t launch_leftmost_deltas(const LeftmostReplaceArgs &a, hipStream_t st);
hipError_t launch_leftmost_starts(const LeftmostReplaceArgs &a, hipStream_t st);
hipError_t launch_leftmost_copy(const LeftmostReplaceArgs &a, hipStream_t st);

}  // namespace ss
