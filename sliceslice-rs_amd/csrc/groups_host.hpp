// groups_host.hpp - the host side of the grouping calls (include/sliceslice_hip_groups.h has THE RULE; ss_groups.hip uses this file).
// Plain C++, no HIP call:
//   groups_table_size     the slots of the hash table of a call over n ranges
//   groups_blocks         its rank blocks
//   groups_scratch_bytes  the temporary device memory it takes, array by array
//   check_groups_flags    NULL, or what is wrong with the flags
#pragma once
#include <cstddef>
#include <cstdint>

namespace ssh {
namespace groups {

constexpr uint64_t kMaxRanges = 0xfffffffeull;          // SS_GROUPS_MAX_RANGES: 2^32 - 2 (0xffffffff is the EMPTY slot)
constexpr uint64_t kBlockRanges = 4096;                 // SS_GROUPS_BLOCK
constexpr uint64_t kMaxSlots = 1ull << 32;              // slots are numbered in 32 bits
constexpr unsigned kNocase = 1u, kWeakHash = 2u;        // SS_GROUPS_NOCASE, SS_GROUPS_WEAK_HASH

// The smallest power of two that is at least 2n (at least 2), but never more than 2^32, the most that 32-bit slot numbers reach:
// 2^32 it is from 2^30 + 1 ranges on, and above 2^31 ranges that is below 2n but still more than n, so a probe sequence always
// meets an empty slot.  With 2^32 slots EVERY 32-bit value is a slot number: none can serve as a marker.  0 for n == 0.
inline uint64_t groups_table_size(uint64_t n)
{
    if (n == 0) return 0;
    uint64_t t = 2;
    while (t < 2 * n && t < kMaxSlots) t <<= 1;
    return t;
}

inline uint64_t groups_blocks(uint64_t n) { return (n + kBlockRanges - 1) / kBlockRanges; }

// [totals: 32][hash: 8 n][rank: 8 blocks][table: 4 T][counter: 4 T][slot: 4 n][block count: 4 blocks]
inline uint64_t groups_scratch_bytes(uint64_t n)
{
    return 32 + 12 * n + 8 * groups_table_size(n) + 12 * groups_blocks(n);
}

inline const char *check_groups_flags(unsigned flags)
{
    if (flags & ~(kNocase | kWeakHash)) return "unknown flag bits (SS_GROUPS_NOCASE and SS_GROUPS_WEAK_HASH are the flags)";
    return nullptr;
}

}  // namespace groups
}  // namespace ssh
