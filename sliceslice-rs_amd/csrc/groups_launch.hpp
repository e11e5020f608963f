// groups_launch.hpp - argument block and host-side entry points of the grouping kernels (groups_kernels.hpp; defined and used in
// ss_groups.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace ss {

constexpr uint32_t kGroupsEmpty = 0xffffffffu;          // a slot that holds no member
constexpr int kGroupsThreads = 256;
constexpr int kGroupsBlock = 4096;                      // SS_GROUPS_BLOCK: ranges per rank block
constexpr int kGroupsLaneMax = 128;                     // SS_GROUPS_LANE_MAX: the longest key one lane hashes and compares alone
constexpr int kGroupsLdsBits = 11;                      // groups_count_kernel: the workgroup's LDS table ...
constexpr int kGroupsLdsSlots = 1 << kGroupsLdsBits;    // ... has 2,048 entries of 12 bytes: SS_GROUPS_LDS_BYTES = 24,576
constexpr int kGroupsLdsProbes = 4;                     // ... and an add that finds no entry in four probes goes to global memory
constexpr int kGroupsFlag = 0, kGroupsEmit = 1;         // groups_rank_kernel

struct GroupsArgs {
    const uint8_t *hay;
    uint64_t len;
    const uint64_t *begin, *end;    // n ranges, clamped to the view by out_clamp (output_host.hpp)
    uint64_t n;
    uint32_t weak;                  // SS_GROUPS_WEAK_HASH
    uint32_t reserved;
    uint64_t tmask;                 // slots - 1
    uint64_t blocks;                // ceil(n / kGroupsBlock)
    // scratch
    uint64_t *totals;               // [0] groups, [1] lanes that found no slot (never: the table is larger than n)
    uint64_t *hash;                 // n
    uint64_t *rank;                 // blocks
    uint32_t *table;                // slots: a member of the slot's group, after the insert kernel its first; or kGroupsEmpty
    uint32_t *counter;              // slots: the members; behind the emit pass the group's number
    uint32_t *slot;                 // n: where range k found its group
    uint32_t *bcount;               // blocks: first members per block
    // results, each may be NULL; first / count / out_* hold `capacity` entries, group holds n
    uint64_t *first, *count, *group;
    uint64_t *out_b, *out_e, *out_n;    // begin / end of the group's first member as given, and its index + 1
    uint64_t capacity;
};

// ceil(n / kGroupsThreads) workgroups of kGroupsThreads lanes
hipError_t launch_groups_hash(const GroupsArgs &a, bool fold, hipStream_t st);
hipError_t launch_groups_insert(const GroupsArgs &a, bool fold, hipStream_t st);
// `blocks` workgroups
hipError_t launch_groups_count(const GroupsArgs &a, hipStream_t st);
hipError_t launch_groups_number(const GroupsArgs &a, hipStream_t st);
// `blocks` workgroups; kGroupsFlag leaves bcount, kGroupsEmit reads rank
hipError_t launch_groups_rank(const GroupsArgs &a, int mode, hipStream_t st);

}  // namespace ss
