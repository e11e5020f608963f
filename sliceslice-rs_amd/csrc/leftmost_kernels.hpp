// leftmost_kernels.hpp - the kernels of the leftmost-longest selection over a needle set's pairs and of the set replace
// (include/sliceslice_hip_leftmost.h; libsliceslice_hip_leftmost.so only: ss_leftmost.hip holds them and their host side).
//
// disjoint_kernels.hpp's scheme with a length per entry.  The list may repeat an offset; the LAST entry of a run of equal offsets is
// the run's candidate (lengths ascend inside a run).  Runs are handled inside the staging, not by compacting the candidates first:
// an entry that is no candidate is transparent - its successor is its neighbour and it counts nothing - and a candidate's
// successor is the FIRST entry at or beyond its end, the first of that run, from which the walk steps to the run's candidate.  A
// run that straddles a block border needs nothing special: its entries in the earlier block are terminals that exit to the next
// entry.  Two facts cut the chain:
//   heads          an entry that stands the list's largest length or more beyond its predecessor (and the first entry) is the first
//                  of its run, and every walk that starts before it lands on it: no earlier candidate reaches beyond it, and a walk
//                  only steps to its neighbour or to an entry at or below the head.  The sufficient form of the issue's fact (c);
//   bounded reach  candidates have distinct offsets, so a candidate's successor lies at most its length in CANDIDATES ahead.  In
//                  entries the bound is that times the longest run, which the primitive does not know, so the searches run over
//                  the rest of the block (twelve steps) and, for a terminal, over the rest of the list.
//
//   leftmost_longest_kernel / _final_kernel  the largest length of the list: one word per block, then one workgroup.
//   leftmost_block_kernel   one workgroup per block of SS_LEFTMOST_BLOCK entries, the offsets staged in LDS.  Every entry finds its
//                           successor inside the block (none: it is a terminal, points at itself, and finds its exit in the whole
//                           list); pointer doubling - twelve rounds, each ended by a barrier - gives every entry the
//                           candidates of the walk that starts at it and the terminal it ends on.  A record (selections << 48 |
//                           exit) is stored for the entries up to the block's first head and for every entry of a block without one.
//   leftmost_chain_kernel   one workgroup: a lane per block with a head hands the block's fixed exit on and walks the head-less blocks
//                           behind it, one record each, until it enters the next block with a head.
//   prefix_kernel           (prefix_kernel.hpp) the selections in front of every block, and their total.
//   leftmost_emit_kernel    the blocks that hold one of the first `capacity` selections build the counts again; the entry and every
//                           head behind it start a walk to the next head, at the rank their counts give them.
//   leftmost_deltas_kernel  per block of selections the sum of (replacement length - needle length), modulo 2^64; prefix_kernel.
//   leftmost_starts_kernel  those differences scanned inside the block in LDS: the output offset of every selection.
//   leftmost_copy_kernel    the grid is over the OUTPUT, output_kernels.hpp's way: one workgroup per chunk of SS_OUTPUT_CHUNK bytes
//                           cut from the 16-byte aligned address at or below d_out.  Two lanes find the chunk's slice of the starts;
//                           every lane owns one 16-byte unit at a time and finds the last selection that starts at or below the
//                           unit's first byte by binary search in that slice.  A unit inside one replacement or one gap of haystack
//                           text is one 16-byte load and ONE 16-byte store; a unit that holds a border is composed in two 64-bit
//                           registers and stored once; only the units cut by d_out's own first and last byte go byte by byte.
// LDS: 48 KiB in the block and the emit kernel (offsets 32, pointers 8, counts 8), the limit; the search for the first head borrows the
// counts' words before they are set.  No workgroup waits for another, no global atomic, the output depends on the input alone.  A
// list that breaks the contract costs nothing but its values: successors lie behind their entry, exits behind their block, and a
// store is made only below a block's own rank plus its own count.
#pragma once
#include "leftmost_launch.hpp"
#include "prefix_kernel.hpp"

namespace ss {

constexpr uint32_t kLmBlock = SS_LEFTMOST_BLOCK;
constexpr int kLmPer = (int)(kLmBlock / kLeftmostThreads);
constexpr uint32_t kLmChunk = SS_OUTPUT_CHUNK;
constexpr int kLmUnits = (int)(kLmChunk / 16 / kLeftmostCopyThreads);
constexpr uint64_t kLmCandidate = 1ull << 63;                   // in a terminal's LDS word: the terminal is a candidate
static_assert(kLmBlock % kLeftmostThreads == 0 && kLmPer == 4 && kLmBlock <= 32768, "local indices are 16-bit, four entries per lane");
static_assert(kLmChunk % (16 * kLeftmostCopyThreads) == 0 && kLmUnits == 4, "a chunk is four units per lane");

__device__ __forceinline__ uint64_t lm_length(const LeftmostArgs &a, uint64_t g) { return a.lengths ? a.lengths[g] : a.rank_len[a.ranks[g]]; }

// the first index k of [lo, hi) with v[k] >= t, else hi
template <class Index>
__device__ __forceinline__ Index lm_lower_bound(const uint64_t *v, Index lo, Index hi, uint64_t t)
{
    while (lo < hi) {
        const Index mid = lo + (hi - lo) / 2;
        if (v[mid] < t) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// the number of entries of v[lo, hi) at or below x, plus lo
__device__ __forceinline__ uint64_t lm_upper_bound(const uint64_t *v, uint64_t lo, uint64_t hi, uint64_t x)
{
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (v[mid] <= x) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// the largest of the lanes' values, in every lane
__device__ __forceinline__ uint64_t lm_block_max(uint64_t m, uint64_t *s_max)
{
    s_max[threadIdx.x] = m;
    __syncthreads();
    for (unsigned k = kLeftmostThreads / 2; k != 0; k >>= 1) {
        if (threadIdx.x < k && s_max[threadIdx.x + k] > s_max[threadIdx.x]) s_max[threadIdx.x] = s_max[threadIdx.x + k];
        __syncthreads();
    }
    return s_max[0];
}

__global__ void __launch_bounds__(kLeftmostThreads) leftmost_longest_kernel(LeftmostArgs a)
{
    __shared__ uint64_t s_max[kLeftmostThreads];
    const uint64_t base = (uint64_t)blockIdx.x * kLmBlock;
    uint64_t m = 0;
#pragma unroll
    for (int i = 0; i < kLmPer; ++i) {
        const uint64_t g = base + threadIdx.x + (uint64_t)i * kLeftmostThreads;
        if (g < a.count) {
            const uint64_t l = lm_length(a, g);
            if (l > m) m = l;
        }
    }
    m = lm_block_max(m, s_max);
    if (threadIdx.x == 0) a.cnt[blockIdx.x] = m;
}

__global__ void __launch_bounds__(kLeftmostThreads) leftmost_longest_final_kernel(LeftmostArgs a)
{
    __shared__ uint64_t s_max[kLeftmostThreads];
    uint64_t m = 0;
    for (uint64_t b = threadIdx.x; b < a.blocks; b += kLeftmostThreads)
        if (a.cnt[b] > m) m = a.cnt[b];
    m = lm_block_max(m, s_max);
    if (threadIdx.x == 0) a.total[1] = m;
}

// Is entry j of the staged block the last of its run of equal offsets?
__device__ __forceinline__ bool lm_candidate(const LeftmostArgs &a, uint64_t base, uint32_t len, const uint64_t *s_off, uint32_t j)
{
    if (j + 1 < len) return s_off[j + 1] != s_off[j];
    const uint64_t g = base + len;
    return g >= a.count || a.offsets[g] != s_off[j];
}

// Does entry j stand `longest` or more beyond its predecessor (or first in the list)?
__device__ __forceinline__ bool lm_head(const LeftmostArgs &a, uint64_t base, const uint64_t *s_off, uint32_t j, uint64_t longest)
{
    if (j == 0 && base == 0) return true;
    const uint64_t prev = j != 0 ? s_off[j - 1] : a.offsets[base - 1], p = s_off[j];
    return p > prev && p - prev >= longest;
}

// The successor of entry j inside the staged block, or `len`: its neighbour where it is no candidate, else the first entry at or
// beyond its end.  *end_at = that end (valid where *reaches).
__device__ __forceinline__ uint32_t lm_successor(const LeftmostArgs &a, uint64_t base, uint32_t len, const uint64_t *s_off, uint32_t j, bool candidate,
                                                 uint64_t *end_at, bool *reaches)
{
    *reaches = true;
    *end_at = s_off[j];
    if (!candidate) return j + 1;
    const uint64_t p = s_off[j], l = lm_length(a, base + j);
    if (p > ~0ull - l) {                                            // (nothing can stand at or beyond p + l)
        *reaches = false;
        return len;
    }
    *end_at = p + l;
    return lm_lower_bound<uint32_t>(s_off, j + 1, len, p + l);
}

// Pointer doubling.  In: s_ptr[j] = the successor of j, or j itself for a terminal; s_cnt[j] = the candidates of [j, s_ptr[j]).
// Out: s_ptr[j] = the terminal the walk from j ends on, s_cnt[j] = the candidates of the walk in front of that terminal.
__device__ __forceinline__ void lm_double(uint32_t len, uint16_t *s_ptr, uint16_t *s_cnt)
{
    for (uint32_t span = 1; span < kLmBlock; span <<= 1) {
        uint16_t np[kLmPer], nc[kLmPer];
        int live = 0;
#pragma unroll
        for (int i = 0; i < kLmPer; ++i) {
            const uint32_t j = threadIdx.x + (uint32_t)i * kLeftmostThreads;
            np[i] = nc[i] = 0;
            if (j < len) {
                const uint16_t p = s_ptr[j], q = s_ptr[p];
                if (q != p) {                                           // (p is no terminal yet)
                    np[i] = q;
                    nc[i] = (uint16_t)(s_cnt[j] + s_cnt[p]);
                    live |= 1 << i;
                }
            }
        }
        __syncthreads();                        // (always twelve rounds: a vote that ends them early would cost LDS beyond the 48 KiB)
#pragma unroll
        for (int i = 0; i < kLmPer; ++i) {
            const uint32_t j = threadIdx.x + (uint32_t)i * kLeftmostThreads;
            if (live & (1 << i)) {
                s_ptr[j] = np[i];
                s_cnt[j] = nc[i];
            }
        }
        __syncthreads();
    }
}

__global__ void __launch_bounds__(kLeftmostThreads) leftmost_block_kernel(LeftmostArgs a)
{
    __shared__ uint64_t s_off[kLmBlock];
    __shared__ uint16_t s_ptr[kLmBlock];
    __shared__ __attribute__((aligned(8))) uint16_t s_cnt[kLmBlock];
    uint32_t *s_head = reinterpret_cast<uint32_t *>(s_cnt);             // (borrowed until the counts are set)
    const uint64_t base = (uint64_t)blockIdx.x * kLmBlock;
    const uint32_t len = a.count - base < kLmBlock ? (uint32_t)(a.count - base) : kLmBlock;
    const uint64_t end = base + len, longest = a.total[1];
    if (threadIdx.x == 0) *s_head = kLeftmostNone;
    for (uint32_t j = threadIdx.x; j < len; j += kLeftmostThreads) s_off[j] = a.offsets[base + j];
    __syncthreads();
    // every entry's successor; a terminal's lies behind the block: its index in the whole list takes the place of its offset in LDS
    uint64_t exit[kLmPer];
    uint16_t ptr[kLmPer], cnt[kLmPer];
    int terminal = 0;
    uint32_t first = kLeftmostNone;
#pragma unroll
    for (int i = 0; i < kLmPer; ++i) {
        const uint32_t j = threadIdx.x + (uint32_t)i * kLeftmostThreads;
        exit[i] = 0;
        ptr[i] = cnt[i] = 0;
        if (j >= len) continue;
        const bool candidate = lm_candidate(a, base, len, s_off, j);
        uint64_t end_at;
        bool reaches;
        const uint32_t succ = lm_successor(a, base, len, s_off, j, candidate, &end_at, &reaches);
        if (succ < len) {
            ptr[i] = (uint16_t)succ;
            cnt[i] = candidate ? 1 : 0;
        } else {
            terminal |= 1 << i;
            ptr[i] = (uint16_t)j;
            uint64_t e = a.count;
            if (!candidate) e = end;                                    // (its neighbour)
            else if (reaches && end < a.count) e = lm_lower_bound<uint64_t>(a.offsets, end, a.count, end_at);
            exit[i] = e | (candidate ? kLmCandidate : 0);
        }
        if (first == kLeftmostNone && lm_head(a, base, s_off, j, longest)) first = j;
    }
    if (first != kLeftmostNone) atomicMin(s_head, first);               // (LDS)
    __syncthreads();
    const uint32_t head = *s_head;
    __syncthreads();
#pragma unroll
    for (int i = 0; i < kLmPer; ++i) {
        const uint32_t j = threadIdx.x + (uint32_t)i * kLeftmostThreads;
        if (j >= len) continue;
        s_ptr[j] = ptr[i];
        s_cnt[j] = cnt[i];
        if (terminal & (1 << i)) s_off[j] = exit[i];
    }
    __syncthreads();
    lm_double(len, s_ptr, s_cnt);
    if (threadIdx.x == 0) a.head[blockIdx.x] = head;
    for (uint32_t j = threadIdx.x; j < len; j += kLeftmostThreads)
        if (head == kLeftmostNone || j <= head) {
            const uint64_t t = s_off[s_ptr[j]];
            a.rec[base + j] = ((uint64_t)s_cnt[j] + (t >> 63)) << kLeftmostExitBits | (t & kLeftmostExitMask);
        }
}

__global__ void __launch_bounds__(kLeftmostThreads) leftmost_chain_kernel(LeftmostArgs a)
{
    for (uint64_t b = threadIdx.x; b < a.blocks; b += kLeftmostThreads) {
        a.entry[b] = b == 0 ? 0u : kLeftmostNone;
        a.cnt[b] = 0;
    }
    __syncthreads();
    for (uint64_t b = threadIdx.x; b < a.blocks; b += kLeftmostThreads) {
        const uint32_t head = a.head[b];
        if (head == kLeftmostNone) continue;
        uint64_t e = a.rec[b * kLmBlock + head] & kLeftmostExitMask;        // behind block b, whichever way it was entered
        while (e < a.count) {
            const uint64_t c = e / kLmBlock;
            if (c <= b) break;                                              // (never where the records are the block kernel's)
            const uint32_t at = (uint32_t)(e % kLmBlock), hc = a.head[c];
            if (hc != kLeftmostNone) {
                a.entry[c] = at <= hc ? at : hc;                            // (at <= hc wherever the list keeps the contract)
                break;
            }
            const uint64_t r = a.rec[e];
            const uint64_t next = r & kLeftmostExitMask;
            a.entry[c] = at;
            a.cnt[c] = r >> kLeftmostExitBits;
            if (next <= e) break;                                           // (likewise)
            e = next;
        }
    }
    __syncthreads();
    for (uint64_t b = threadIdx.x; b < a.blocks; b += kLeftmostThreads) {
        const uint32_t head = a.head[b], at = a.entry[b];
        if (head != kLeftmostNone && at != kLeftmostNone) a.cnt[b] = a.rec[b * kLmBlock + at] >> kLeftmostExitBits;
    }
}

__global__ void __launch_bounds__(kLeftmostThreads) leftmost_emit_kernel(LeftmostArgs a)
{
    __shared__ uint64_t s_off[kLmBlock];
    __shared__ uint16_t s_ptr[kLmBlock], s_cnt[kLmBlock];
    const uint32_t at = a.entry[blockIdx.x];
    const uint64_t rank = a.rank[blockIdx.x], want = a.cnt[blockIdx.x];
    if (at == kLeftmostNone || want == 0 || rank >= a.capacity) return;    // (workgroup-uniform)
    const uint64_t base = (uint64_t)blockIdx.x * kLmBlock;
    const uint32_t len = a.count - base < kLmBlock ? (uint32_t)(a.count - base) : kLmBlock;
    const uint64_t longest = a.total[1];
    if (at >= len) return;                                                  // (never; the entry is an index of this block)
    for (uint32_t j = threadIdx.x; j < len; j += kLeftmostThreads) s_off[j] = a.offsets[base + j];
    __syncthreads();
    for (uint32_t j = threadIdx.x; j < len; j += kLeftmostThreads) {
        const bool candidate = lm_candidate(a, base, len, s_off, j);
        uint64_t end_at;
        bool reaches;
        const uint32_t succ = lm_successor(a, base, len, s_off, j, candidate, &end_at, &reaches);
        s_ptr[j] = (uint16_t)(succ < len ? succ : j);
        s_cnt[j] = (uint16_t)(succ < len && candidate ? 1 : 0);
    }
    __syncthreads();
    lm_double(len, s_ptr, s_cnt);
    const uint32_t from_entry = s_cnt[at];
    for (uint32_t j = threadIdx.x; j < len; j += kLeftmostThreads) {
        if (j < at || (j != at && !lm_head(a, base, s_off, j, longest))) continue;
        uint32_t r = from_entry - s_cnt[j], k = j;                          // the entry and every head behind it are on its walk
        do {
            const bool candidate = lm_candidate(a, base, len, s_off, k);
            if (candidate) {
                if (r >= want || rank + r >= a.capacity) break;
                if (a.out) a.out[rank + r] = s_off[k];
                if (a.which) a.which[rank + r] = base + k;
                if (a.out_ranks) a.out_ranks[rank + r] = a.ranks[base + k];
                ++r;
            }
            uint64_t end_at;
            bool reaches;
            k = lm_successor(a, base, len, s_off, k, candidate, &end_at, &reaches);
        } while (k < len && !lm_head(a, base, s_off, k, longest));
    }
}

// ---- the set replace --------------------------------------------------------------------------------------------------------------

// replacement length - needle length of selection i, modulo 2^64
__device__ __forceinline__ uint64_t lm_delta(const LeftmostReplaceArgs &a, uint64_t i)
{
    const LeftmostRank r = a.table[a.sel_rank[i]];
    return r.rep_len - r.needle_len;
}

__global__ void __launch_bounds__(kLeftmostThreads) leftmost_deltas_kernel(LeftmostReplaceArgs a)
{
    __shared__ uint64_t s_sum[kLeftmostThreads];
    const uint64_t base = (uint64_t)blockIdx.x * kLmBlock;
    uint64_t sum = 0;
#pragma unroll
    for (int k = 0; k < kLmPer; ++k) {
        const uint64_t i = base + threadIdx.x + (uint64_t)k * kLeftmostThreads;
        if (i < a.nsel) sum += lm_delta(a, i);
    }
    s_sum[threadIdx.x] = sum;
    __syncthreads();
    for (unsigned k = kLeftmostThreads / 2; k != 0; k >>= 1) {
        if (threadIdx.x < k) s_sum[threadIdx.x] += s_sum[threadIdx.x + k];
        __syncthreads();
    }
    if (threadIdx.x == 0) a.sum[blockIdx.x] = s_sum[0];
}

__global__ void __launch_bounds__(kLeftmostThreads) leftmost_starts_kernel(LeftmostReplaceArgs a)
{
    __shared__ uint64_t s_delta[kLmBlock];
    __shared__ uint64_t s_run[kLeftmostThreads];
    const uint64_t base = (uint64_t)blockIdx.x * kLmBlock;
    const uint32_t n = a.nsel - base < kLmBlock ? (uint32_t)(a.nsel - base) : kLmBlock;
#pragma unroll
    for (int k = 0; k < kLmPer; ++k) {
        const uint32_t j = threadIdx.x + (uint32_t)k * kLeftmostThreads;
        s_delta[j] = j < n ? lm_delta(a, base + j) : 0;
    }
    __syncthreads();
    // lane t owns the differences kLmPer * t ..; the lanes' sums are scanned (Hillis-Steele, inclusive), then every lane ranks its own
    uint64_t v[kLmPer], sum = 0;
#pragma unroll
    for (int k = 0; k < kLmPer; ++k) {
        v[k] = s_delta[threadIdx.x * kLmPer + k];
        sum += v[k];
    }
    s_run[threadIdx.x] = sum;
    __syncthreads();
    for (int k = 1; k < kLeftmostThreads; k <<= 1) {
        const uint64_t w = threadIdx.x >= (unsigned)k ? s_run[threadIdx.x - k] : 0ull;
        __syncthreads();
        s_run[threadIdx.x] += w;
        __syncthreads();
    }
    uint64_t r = s_run[threadIdx.x] - sum;
#pragma unroll
    for (int k = 0; k < kLmPer; ++k) {
        s_delta[threadIdx.x * kLmPer + k] = r;
        r += v[k];
    }
    __syncthreads();
    const uint64_t rank = a.rank[blockIdx.x];
#pragma unroll
    for (int k = 0; k < kLmPer; ++k) {
        const uint32_t j = threadIdx.x + (uint32_t)k * kLeftmostThreads;
        if (j < n) a.starts[base + j] = a.sel[base + j] + rank + s_delta[j];
    }
}

// 16 bytes at any alignment in one global load: the target allows unaligned vector accesses
typedef uint32_t lm_u32x4_unaligned __attribute__((ext_vector_type(4), aligned(1)));
__device__ __forceinline__ uint4 lm_load16(const uint8_t *src)
{
    const lm_u32x4_unaligned v = *reinterpret_cast<const lm_u32x4_unaligned *>(src);
    return make_uint4(v.x, v.y, v.z, v.w);
}

// byte `t` (0 .. 15) of the unit held in (w0, w1)
__device__ __forceinline__ void lm_put(uint64_t &w0, uint64_t &w1, unsigned t, uint8_t byte)
{
    if (t < 8) w0 |= (uint64_t)byte << (8 * t);
    else w1 |= (uint64_t)byte << (8 * (t - 8));
}

// the first m (1 .. 16 - t) bytes of v at the bytes t .. of the unit
__device__ __forceinline__ void lm_put_bytes(uint64_t &w0, uint64_t &w1, unsigned t, unsigned m, uint4 v)
{
    uint64_t v0 = v.x | (uint64_t)v.y << 32, v1 = v.z | (uint64_t)v.w << 32;
    if (m < 8) {
        v0 &= (1ull << (8 * m)) - 1;
        v1 = 0;
    } else if (m < 16) {
        v1 &= (1ull << (8 * (m - 8))) - 1;
    }
    if (t >= 8) {
        v1 = v0 << (8 * (t - 8));
        v0 = 0;
    } else if (t != 0) {
        v1 = v1 << (8 * t) | v0 >> (64 - 8 * t);
        v0 <<= 8 * t;
    }
    w0 |= v0;
    w1 |= v1;
}

__global__ void __launch_bounds__(kLeftmostCopyThreads) leftmost_copy_kernel(LeftmostReplaceArgs a)
{
    __shared__ uint64_t s_slice[2];
    const uint64_t q0 = (uint64_t)blockIdx.x * kLmChunk;
    const uint64_t qlo = q0 > a.out_lo ? q0 : a.out_lo, qhi = q0 + kLmChunk < a.out_hi ? q0 + kLmChunk : a.out_hi;
    if (qlo >= qhi) return;                                             // (workgroup-uniform; the host launches no such chunk)
    if (threadIdx.x < 2) {
        // the selections that start at or below the chunk's first and last byte
        const uint64_t o = (threadIdx.x == 0 ? qlo : qhi - 1) - a.out_lo;
        s_slice[threadIdx.x] = lm_upper_bound(a.starts, 0, a.nsel, o);
    }
    __syncthreads();
    const uint64_t r0 = s_slice[0], r1 = s_slice[1], total = a.out_hi - a.out_lo;
#pragma unroll 1
    for (int k = 0; k < kLmUnits; ++k) {
        const uint64_t u = q0 + ((uint64_t)threadIdx.x + (uint64_t)k * kLeftmostCopyThreads) * 16;
        const uint64_t lo = u > qlo ? u : qlo, hi = u + 16 < qhi ? u + 16 : qhi;
        if (lo >= hi) continue;
        const bool whole = hi - lo == 16;
        uint64_t idx = lm_upper_bound(a.starts, r0, r1, lo - a.out_lo);  // the selections that start at or below the unit's first byte
        uint64_t w0 = 0, w1 = 0, q = lo;
        while (q < hi) {                                                // field by field: each adds at least one byte
            const uint64_t oo = q - a.out_lo;
            while (idx < a.nsel && a.starts[idx] <= oo) ++idx;          // (selections that contribute no byte)
            const uint64_t next = idx < a.nsel ? a.starts[idx] : total;
            const uint8_t *src;
            uint64_t avail;
            bool sixteen;                                               // sixteen bytes can be loaded at src
            if (idx == 0) {                                             // the text in front of the first selection
                src = a.hay + oo;
                avail = next - oo;
                sixteen = oo + 16 <= a.len;
                if (oo >= a.len || avail > a.len - oo) avail = 0;       // (never: it is text of the view)
            } else {
                const LeftmostRank r = a.table[a.sel_rank[idx - 1]];
                const uint64_t d = oo - a.starts[idx - 1];
                if (d < r.rep_len) {
                    src = a.blob + r.rep_off + d;                       // (the blob is padded)
                    avail = r.rep_len - d;
                    sixteen = true;
                } else {
                    const uint64_t h = a.sel[idx - 1] + r.needle_len + (d - r.rep_len);
                    src = a.hay + h;
                    avail = next - oo;
                    sixteen = h <= a.len && a.len - h >= 16;
                    if (h >= a.len || avail > a.len - h) avail = 0;     // (never: the gap is text of the view)
                }
            }
            const unsigned t = (unsigned)(q - u), room = (unsigned)(hi - q);
            if (avail == 0) {                                           // (an inconsistent list: the byte stays 0, nothing is loaded)
                ++q;
                continue;
            }
            if (whole && q == lo && avail >= 16 && sixteen) {           // wholly inside one replacement or one gap
                const uint4 v = lm_load16(src);
                w0 = v.x | (uint64_t)v.y << 32;
                w1 = v.z | (uint64_t)v.w << 32;
                break;
            }
            const unsigned m = avail < room ? (unsigned)avail : room;
            if (sixteen) {
                lm_put_bytes(w0, w1, t, m, lm_load16(src));
            } else {
                for (unsigned j = 0; j < m; ++j) lm_put(w0, w1, t + j, src[j]);
            }
            q += m;
        }
        if (whole) {
            *reinterpret_cast<uint4 *>(a.out_base + u) = make_uint4((uint32_t)w0, (uint32_t)(w0 >> 32), (uint32_t)w1, (uint32_t)(w1 >> 32));
        } else {
            for (uint64_t b = lo; b < hi; ++b) {                        // a unit cut by d_out's own first or last byte
                const unsigned t = (unsigned)(b - u);
                a.out_base[b] = (uint8_t)((t < 8 ? w0 : w1) >> (8 * (t & 7)));
            }
        }
    }
}

}  // namespace ss
