// disjoint_launch.hpp - argument blocks and host-side entry points of the selection and the replace kernels
// (disjoint_kernels.hpp; defined and used in ss_disjoint.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "../../include/sliceslice_hip_disjoint.h"

namespace ss {

constexpr int kDisjointThreads = 1024;                          // lanes per workgroup of the block and the emit kernel
constexpr uint32_t kDisjointNone = 0xffffffffu;                 // head: the block holds no head; entry: no chain enters the block
constexpr int kDisjointExitBits = 48;                           // a record: selections << 48 | exit
constexpr uint64_t kDisjointExitMask = (1ull << kDisjointExitBits) - 1;

struct DisjointArgs {
    const uint64_t *offsets;    // strictly ascending (the caller's contract)
    uint64_t count, n;
    uint64_t blocks;            // ceil(count / SS_DISJOINT_BLOCK)
    // scratch
    uint64_t *rec;              // `count` records: the selections of the walk that enters its block at this entry, and its exit (the
                                // global index of the first entry at or beyond the last selected one + n); written for the entries
                                // up to the block's first head, for every entry of a block without one
    uint32_t *head;             // per block: the local index of its first head, or kDisjointNone
    uint32_t *entry;            // per block: the local index at which the chain enters it, or kDisjointNone (skipped whole)
    uint64_t *cnt;              // per block: its selections
    uint64_t *rank;             // per block: the selections in front of it
    uint64_t *total;
    // emit
    uint64_t *out;
    uint64_t capacity;
};

struct ReplaceArgs {
    const uint8_t *base;        // the 16-byte aligned address at or below the view
    uint64_t lo, hi;            // the view is base[lo, hi)
    uint64_t parts;             // parts of SS_CONTEXT_PART_BYTES from `base`
    const uint64_t *sel;        // the selected occurrences, ascending offsets of the view
    uint64_t nsel;
    uint64_t n;                 // the needle's length
    const uint8_t *rep;         // the replacement, in device memory
    uint64_t rep_len;
    uint8_t *out;
};

// ceil(count / SS_DISJOINT_BLOCK) workgroups of kDisjointThreads lanes
hipError_t launch_disjoint_block(const DisjointArgs &a, hipStream_t st);
// one workgroup: every block's entry and selections; then the prefix over the selections (prefix_kernel.hpp) -> rank, *total
hipError_t launch_disjoint_chain(const DisjointArgs &a, hipStream_t st);
hipError_t launch_disjoint_emit(const DisjointArgs &a, hipStream_t st);
// `parts` workgroups of kBlock lanes
hipError_t launch_replace(const ReplaceArgs &a, hipStream_t st);

}  // namespace ss
