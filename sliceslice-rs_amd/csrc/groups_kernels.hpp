// groups_kernels.hpp - the kernels that group equal keys (include/sliceslice_hip_groups.h has THE RULE; libsliceslice_hip_groups.so
// only: ss_groups.hip holds them and their host side).  One lane per range everywhere, kGroupsThreads lanes per workgroup.
//
//   groups_hash_kernel    hash[k]: 64 bits of the key's bytes and length.  The key's bytes come as ALIGNED dwords, from the one that
//                         holds its first byte to the one that holds its last, shifted together in registers: no load touches a
//                         dword without a byte of the key, so none touches a 16-byte block without a byte of the view.  The last
//                         dword's bytes beyond the key are cleared and the fold, where asked, is applied to the register.  A key of
//                         at most kGroupsLaneMax bytes is hashed by its own lane, one load per dword.  The wave then takes its
//                         longer keys one after the other, lane l the dwords l, l + 64, ...: every dword is mixed with its index,
//                         the lanes' sums are added up - a sum, so the order of the lanes does not matter - and mixed with the
//                         length.  Equal keys have equal lengths and so take the same path.
//                         WHY 128: a step of the wave path costs two loads and a twelve-step sum, about what two dwords cost a
//                         lane, but its steps are serial over the wave's long keys, while the lane loop runs as long as the
//                         wave's longest short key.  With every lane long - lines of text - 64 wave steps stand against
//                         len / 4 lane steps: the wave path wins above some hundred bytes, and text lines (41 bytes on average in
//                         the manual, few above 80) stay below it; with one long key in a wave it wins much earlier.  128 keeps
//                         tokens and text lines private and bounds a lane's loop at 32 dwords.  This is reasoning: NOBODY HAS MEASURED
//                         keys of 100 to 1,000 bytes on either side of the threshold.
//   groups_insert_kernel  the table: open addressing, linear probing, slots of 32 bits that hold kGroupsEmpty or the index of a
//                         member of the slot's group.  A lane reads its slot with a relaxed agent-scope atomic load (a plain load
//                         may be served from the CU's L1, which other CUs' atomics never refresh).  EMPTY: one compare-and-swap of
//                         its own index; where that loses it has read the winner and goes on as for an occupied slot.  OCCUPIED by
//                         v: the stored hashes first, then the lengths, then the bytes - by the lane alone up to kGroupsLaneMax
//                         bytes, above that by the whole wave, which serves the lanes that ask in turn.  Equal: the lane joins - an
//                         atomic min of its index, issued only where the value it read is above it - and records the slot.
//                         Unequal: the next slot.
//                         WHY THE LOOP CANNOT HANG: no lane waits for anything another lane does.  Every turn of the loop ends, for
//                         every lane still in it, with the lane done (swap won, or joined) or one slot further; the probes of a
//                         lane are counted and end at the table's size, which cannot be reached because the table has more slots
//                         than there are ranges and a slot, once taken, keeps its group for good (it never becomes empty, and a
//                         min replaces a member by a member of the same group, so whatever index a lane reads from a slot is
//                         good for the comparison).  Two equal keys start at the same slot and pass the same occupied slots, so
//                         they meet in the first slot that is empty or theirs.  After the kernel a slot holds the smallest index
//                         of its group whatever the arrival order was.
//   groups_count_kernel   one add per member into the slot's counter, combined twice before it leaves the CU.  A workgroup takes a
//                         block of kGroupsBlock ranges, sixteen rounds of one range per lane.  Inside the wave the first lane still
//                         pending names its slot, the lanes with that slot are counted by one ballot, and the leader adds their
//                         number - not to global memory but to a workgroup-private table in LDS, kGroupsLdsSlots entries of
//                         (slot | occupied bit, count) found by at most kGroupsLdsProbes probes; a leader that finds no entry adds to
//                         global memory itself.  Behind a barrier every occupied entry is flushed with ONE add: a token that is
//                         5 % of all tokens costs one global add per 4,096 ranges instead of one per wave.
//   A SLOT NUMBER IS NEVER A MARKER: with 2^32 slots every 32-bit value is a slot.  kGroupsEmpty marks a table ENTRY that holds no
//                         member - members are indices below 2^32 - 2 - and nothing else; a range without a slot is one with
//                         k >= n, or one that found none, which fails the call through totals[1].
//   groups_rank_kernel    a range is a first member when its slot holds its own index.  kGroupsFlag: the first members of a block
//                         of kGroupsBlock ranges; prefix_kernel (prefix_kernel.hpp) ranks the blocks; kGroupsEmit: the same
//                         ballots again, and every first member, ranked inside its wave by the lanes below it and inside the
//                         block by the waves in front, writes its results at its rank and leaves its rank - the group's number -
//                         in the slot's counter.
//   groups_number_kernel  group[k] = the number in the counter of range k's slot.
// Atomics are ordinary vector atomics on global memory.  Counts are sums of integers and ranks are prefix sums in index order: the
// output depends on the input alone.
#pragma once
#include "groups_launch.hpp"
#include "prefix_kernel.hpp"
#include "scan_filters.hpp"

#ifndef SS_OUTPUT_FN
#define SS_OUTPUT_FN __host__ __device__ __forceinline__
#endif
#include "output_host.hpp"

namespace ss {

static_assert(kGroupsBlock == 16 * kGroupsThreads && kGroupsThreads == 4 * kWave, "a rank block is sixteen rounds of four waves");

constexpr uint64_t kGroupsSeed = 0x9e3779b97f4a7c15ull, kGroupsMulA = 0xff51afd7ed558ccdull, kGroupsMulB = 0xc4ceb9fe1a85ec53ull;

__device__ __forceinline__ uint64_t groups_mix(uint64_t x)
{
    x ^= x >> 33;
    x *= kGroupsMulA;
    x ^= x >> 33;
    x *= kGroupsMulB;
    return x ^ (x >> 33);
}

// the key hay[b, b + len), len != 0, as aligned dwords: p[0] holds its first byte, p[last] its last
struct GroupsKey {
    const uint32_t *p;
    uint32_t sh;            // bits the key's first byte stands above bit 0 of p[0]
    uint64_t last;
    uint64_t len;
};

__device__ __forceinline__ GroupsKey groups_key(const uint8_t *hay, uint64_t b, uint64_t len)
{
    const uintptr_t at = reinterpret_cast<uintptr_t>(hay + b);
    GroupsKey k;
    k.p = reinterpret_cast<const uint32_t *>(at & ~(uintptr_t)3);
    k.sh = (uint32_t)(at & 3) * 8u;
    k.last = ((at & 3) + len - 1) >> 2;
    k.len = len;
    return k;
}

// bytes 4 i .. 4 i + 3 of the key (4 i < len), those beyond it zero, folded where asked; `w` is p[i], `nx` p[i + 1] or anything
template <bool FOLD>
__device__ __forceinline__ uint32_t groups_shape(const GroupsKey &k, uint64_t i, uint32_t w, uint32_t nx)
{
    uint32_t d = (uint32_t)((((uint64_t)nx << 32) | w) >> k.sh);
    const uint64_t rem = k.len - 4 * i;
    if (rem < 4) d &= (1u << (8 * (uint32_t)rem)) - 1u;
    return FOLD ? fold_ascii4(d) : d;
}

// ... at any i: two loads, the second only where p[i + 1] holds a byte of the key
template <bool FOLD>
__device__ __forceinline__ uint32_t groups_dword(const GroupsKey &k, uint64_t i)
{
    const uint32_t w = k.p[i];
    const uint32_t nx = k.sh != 0 && i < k.last ? k.p[i + 1] : 0u;
    return groups_shape<FOLD>(k, i, w, nx);
}

// ... one after the other: one load per dword
template <bool FOLD>
struct GroupsReader {
    GroupsKey k;
    uint32_t w;
    uint64_t i;
    __device__ __forceinline__ GroupsReader(const uint8_t *hay, uint64_t b, uint64_t len) : k(groups_key(hay, b, len)), w(k.p[0]), i(0) {}
    __device__ __forceinline__ uint32_t next()
    {
        const uint32_t nx = i < k.last ? k.p[i + 1] : 0u;
        const uint32_t d = groups_shape<FOLD>(k, i, w, nx);
        w = nx;
        ++i;
        return d;
    }
};

// a key of 1 .. kGroupsLaneMax bytes, by its lane
template <bool FOLD>
__device__ __forceinline__ uint64_t groups_hash_lane(const uint8_t *hay, uint64_t b, uint64_t len)
{
    uint64_t h = kGroupsSeed ^ (len * kGroupsMulA);
    GroupsReader<FOLD> r(hay, b, len);
    const uint32_t ndw = (uint32_t)((len + 3) >> 2);
    for (uint32_t i = 0; i < ndw; ++i) {
        h = (h ^ r.next()) * kGroupsMulB;
        h ^= h >> 32;
    }
    return groups_mix(h);
}

__device__ __forceinline__ uint64_t groups_wave_sum(uint64_t v)
{
#pragma unroll
    for (int k = 1; k < kWave; k <<= 1) v += __shfl_xor(v, k, kWave);
    return v;
}

// a longer key, by the whole wave; the arguments are the same in every lane, and so is the answer
template <bool FOLD>
__device__ __forceinline__ uint64_t groups_hash_wave(const uint8_t *hay, uint64_t b, uint64_t len, unsigned lane)
{
    const GroupsKey k = groups_key(hay, b, len);
    const uint64_t ndw = (len + 3) >> 2;
    uint64_t acc = 0;
    for (uint64_t i = lane; i < ndw; i += kWave) acc += groups_mix((uint64_t)groups_dword<FOLD>(k, i) * kGroupsMulB + (i + 1) * kGroupsSeed);
    return groups_mix(groups_wave_sum(acc) ^ (len * kGroupsMulA));
}

// hay[x, x + len) == hay[y, y + len), 1 <= len <= kGroupsLaneMax, by the lane
template <bool FOLD>
__device__ __forceinline__ bool groups_equal_lane(const uint8_t *hay, uint64_t x, uint64_t y, uint64_t len)
{
    GroupsReader<FOLD> p(hay, x, len), q(hay, y, len);
    const uint32_t ndw = (uint32_t)((len + 3) >> 2);
    for (uint32_t i = 0; i < ndw; ++i)
        if (p.next() != q.next()) return false;
    return true;
}

// ... of any length, by the whole wave: 256 bytes of each key per step, and it stops at the first step that differs
template <bool FOLD>
__device__ __forceinline__ bool groups_equal_wave(const uint8_t *hay, uint64_t x, uint64_t y, uint64_t len, unsigned lane)
{
    const GroupsKey p = groups_key(hay, x, len), q = groups_key(hay, y, len);
    const uint64_t ndw = (len + 3) >> 2;
    for (uint64_t i0 = 0; i0 < ndw; i0 += kWave) {
        const uint64_t i = i0 + lane;
        const bool differs = i < ndw && groups_dword<FOLD>(p, i) != groups_dword<FOLD>(q, i);
        if (__builtin_amdgcn_ballot_w64(differs) != 0) return false;
    }
    return true;
}

template <bool FOLD>
__global__ void __launch_bounds__(kGroupsThreads) groups_hash_kernel(GroupsArgs a)
{
    const uint64_t k = (uint64_t)blockIdx.x * kGroupsThreads + threadIdx.x;
    const unsigned lane = threadIdx.x & (kWave - 1);
    const bool live = k < a.n;
    uint64_t b = 0, e = 0;
    if (live) out_clamp(a.begin[k], a.end[k], a.len, &b, &e);
    const uint64_t len = e - b;
    uint64_t h = kGroupsSeed;                                                   // (the empty key)
    if (a.weak) {
        h = len & 3;
    } else {
        if (live && len != 0 && len <= (uint64_t)kGroupsLaneMax) h = groups_hash_lane<FOLD>(a.hay, b, len);
        uint64_t m = __builtin_amdgcn_ballot_w64(live && len > (uint64_t)kGroupsLaneMax);
        while (m != 0) {
            const int src = __builtin_ctzll(m);
            m &= m - 1;
            const uint64_t hw = groups_hash_wave<FOLD>(a.hay, __shfl(b, src, kWave), __shfl(len, src, kWave), lane);
            if ((int)lane == src) h = hw;
        }
    }
    if (live) a.hash[k] = h;
}

template <bool FOLD>
__global__ void __launch_bounds__(kGroupsThreads) groups_insert_kernel(GroupsArgs a)
{
    const uint64_t k = (uint64_t)blockIdx.x * kGroupsThreads + threadIdx.x;
    const unsigned lane = threadIdx.x & (kWave - 1);
    bool active = k < a.n;
    uint64_t b = 0, e = 0, h = 0;
    if (active) {
        out_clamp(a.begin[k], a.end[k], a.len, &b, &e);
        h = a.hash[k];
    }
    const uint64_t len = e - b;
    uint64_t slot = h & a.tmask, probes = 0;
    uint32_t mine = 0;                                                          // (a lane that finds no slot fails the call)
    while (__builtin_amdgcn_ballot_w64(active) != 0) {
        bool ask = false, equal = false;
        uint64_t vb = 0;
        uint32_t v = kGroupsEmpty;
        if (active) {
            v = __hip_atomic_load(&a.table[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (v == kGroupsEmpty) {
                uint32_t seen = kGroupsEmpty;
                if (__hip_atomic_compare_exchange_strong(&a.table[slot], &seen, (uint32_t)k, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) {
                    mine = (uint32_t)slot;
                    active = false;
                } else {
                    v = seen;                                                   // (the winner, or whoever lowered it since)
                }
            }
            if (active && a.hash[v] == h) {
                uint64_t ve;
                out_clamp(a.begin[v], a.end[v], a.len, &vb, &ve);
                if (ve - vb == len) {
                    if (vb == b || len == 0) equal = true;
                    else if (len <= (uint64_t)kGroupsLaneMax) equal = groups_equal_lane<FOLD>(a.hay, b, vb, len);
                    else ask = true;
                }
            }
        }
        uint64_t m = __builtin_amdgcn_ballot_w64(ask);
        while (m != 0) {                                                        // the wave serves the lanes with long keys in turn
            const int src = __builtin_ctzll(m);
            m &= m - 1;
            const bool eq = groups_equal_wave<FOLD>(a.hay, __shfl(b, src, kWave), __shfl(vb, src, kWave), __shfl(len, src, kWave), lane);
            if ((int)lane == src) equal = eq;
        }
        if (active) {
            if (equal) {
                if ((uint32_t)k < v) (void)__hip_atomic_fetch_min(&a.table[slot], (uint32_t)k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                mine = (uint32_t)slot;
                active = false;
            } else {
                slot = (slot + 1) & a.tmask;
                if (++probes > a.tmask) {                                       // every slot seen (never: the table outnumbers the ranges)
                    (void)__hip_atomic_fetch_add(&a.totals[1], 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    active = false;
                }
            }
        }
    }
    if (k < a.n) a.slot[k] = mine;
}

__global__ void __launch_bounds__(kGroupsThreads) groups_count_kernel(GroupsArgs a)
{
    __shared__ unsigned long long s_key[kGroupsLdsSlots];                       // 0, or the slot | 1 << 32
    __shared__ uint32_t s_count[kGroupsLdsSlots];
    constexpr int kRounds = kGroupsBlock / kGroupsThreads;
    const unsigned lane = threadIdx.x & (kWave - 1);
    for (unsigned i = threadIdx.x; i < (unsigned)kGroupsLdsSlots; i += kGroupsThreads) {
        s_key[i] = 0ull;
        s_count[i] = 0u;
    }
    __syncthreads();
    const uint64_t base = (uint64_t)blockIdx.x * kGroupsBlock;
#pragma unroll 1
    for (int r = 0; r < kRounds; ++r) {
        const uint64_t k = base + (uint64_t)r * kGroupsThreads + threadIdx.x;
        bool pending = k < a.n;
        const uint32_t s = pending ? a.slot[k] : 0u;
        uint64_t m;
        while ((m = __builtin_amdgcn_ballot_w64(pending)) != 0) {
            const int leader = __builtin_ctzll(m);
            const uint32_t ls = (uint32_t)__shfl((int)s, leader, kWave);
            const bool same = pending && s == ls;
            const uint64_t members = __builtin_amdgcn_ballot_w64(same);
            if ((int)lane == leader) {
                const uint32_t add = (uint32_t)__builtin_popcountll(members);
                const unsigned long long key = (1ull << 32) | ls;
                uint32_t h = (ls * 0x9e3779b1u) >> (32 - kGroupsLdsBits);
                bool placed = false;
                for (int p = 0; p < kGroupsLdsProbes && !placed; ++p) {
                    const unsigned long long seen = atomicCAS(&s_key[h], 0ull, key);
                    if (seen == 0ull || seen == key) {
                        atomicAdd(&s_count[h], add);
                        placed = true;
                    } else {
                        h = (h + 1) & (uint32_t)(kGroupsLdsSlots - 1);
                    }
                }
                if (!placed) (void)__hip_atomic_fetch_add(&a.counter[ls], add, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            pending = pending && !same;
        }
    }
    __syncthreads();
    for (unsigned i = threadIdx.x; i < (unsigned)kGroupsLdsSlots; i += kGroupsThreads) {
        const unsigned long long key = s_key[i];
        if (key != 0ull) (void)__hip_atomic_fetch_add(&a.counter[(uint32_t)key], s_count[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

template <int MODE>
__global__ void __launch_bounds__(kGroupsThreads) groups_rank_kernel(GroupsArgs a)
{
    __shared__ uint32_t s_wave[kGroupsThreads / kWave];
    constexpr int kRounds = kGroupsBlock / kGroupsThreads;
    const unsigned lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    const uint64_t base = (uint64_t)blockIdx.x * kGroupsBlock + (uint64_t)wave * (kRounds * kWave);
    uint64_t firsts[kRounds];
    uint32_t slots[kRounds];
    uint32_t sum = 0;
#pragma unroll
    for (int r = 0; r < kRounds; ++r) {
        const uint64_t k = base + (uint64_t)r * kWave + lane;
        bool f = false;
        slots[r] = 0;
        if (k < a.n) {
            slots[r] = a.slot[k];
            f = a.table[slots[r]] == (uint32_t)k;
        }
        firsts[r] = __builtin_amdgcn_ballot_w64(f);
        sum += (uint32_t)__builtin_popcountll(firsts[r]);
    }
    if (lane == 0) s_wave[wave] = sum;
    __syncthreads();
    if (MODE == kGroupsFlag) {
        if (threadIdx.x == 0) a.bcount[blockIdx.x] = s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
        return;
    }
    uint64_t j0 = a.rank[blockIdx.x];
    for (unsigned w = 0; w < wave; ++w) j0 += s_wave[w];
    const uint64_t below = (1ull << lane) - 1;
#pragma unroll
    for (int r = 0; r < kRounds; ++r) {
        if ((firsts[r] >> lane) & 1) {
            const uint64_t k = base + (uint64_t)r * kWave + lane;
            const uint64_t j = j0 + (uint64_t)__builtin_popcountll(firsts[r] & below);
            if (j < a.capacity) {
                if (a.first) a.first[j] = k;
                if (a.count) a.count[j] = a.counter[slots[r]];
                if (a.out_b) a.out_b[j] = a.begin[k];
                if (a.out_e) a.out_e[j] = a.end[k];
                if (a.out_n) a.out_n[j] = k + 1;
            }
            a.counter[slots[r]] = (uint32_t)j;                                  // (no other lane reads or writes this counter here)
        }
        j0 += (uint64_t)__builtin_popcountll(firsts[r]);
    }
}

__global__ void __launch_bounds__(kGroupsThreads) groups_number_kernel(GroupsArgs a)
{
    const uint64_t k = (uint64_t)blockIdx.x * kGroupsThreads + threadIdx.x;
    if (k >= a.n) return;
    a.group[k] = a.counter[a.slot[k]];
}

}  // namespace ss
