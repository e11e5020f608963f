// disjoint_kernels.hpp - the kernels of the non-overlapping selection and of replace (include/sliceslice_hip_disjoint.h;
// libsliceslice_hip_disjoint.so only: ss_disjoint.hip holds them and their host side).
//
// The greedy selection is a chain: whether offset j is taken depends on which offset before it was taken.  Two facts cut it:
//   run heads      an offset whose predecessor lies n or more behind it (and the first offset) is selected whatever came earlier; a
//                  chain that stands in front of a head always lands on it, so every chain re-synchronises there;
//   bounded reach  offsets are distinct, so the successor of entry j - the first entry at or beyond offsets[j] + n - has index at
//                  most j + n.
//
//   disjoint_block_kernel  one workgroup per block of SS_DISJOINT_BLOCK offsets, staged in LDS.  Every entry finds its successor inside
//                          the block by binary search (none: it is a terminal, and finds its successor in the whole list); pointer
//                          doubling over the successors - twelve rounds at most, each ended by a barrier - gives every entry the
//                          number of selections of the walk that starts at it and the terminal that walk ends on.  A record
//                          (selections << 48 | exit) is stored for the entries up to the block's first head, whose exit no longer
//                          depends on how the block was entered, and for every entry of a block without a head.
//   disjoint_chain_kernel  one workgroup: a lane per block with a head hands the block's fixed exit on and walks the head-less blocks
//                          behind it, one record each, until it enters the next block with a head.  A block whose entry lies beyond
//                          its end is skipped whole.  Then every block with a head reads the record at its entry.
//   prefix_kernel          (prefix_kernel.hpp) the selections in front of every block, and their total.
//   disjoint_emit_kernel   the blocks that hold one of the first `capacity` selections build the successors and the counts again; the
//                          entry and every head behind it start a walk to the next head, at the rank their counts give them.
//   replace_kernel         one workgroup per part of SS_CONTEXT_PART_BYTES of the view: 16 bytes per lane and load, the number of
//                          selected occurrences at or below a byte by binary search inside the part's slice of the list, a byte
//                          outside every occurrence stored at its position shifted by that number, the replacement stored by the lane
//                          that owns an occurrence's first byte.
// No workgroup waits for another inside a kernel, no global atomic, the output depends on the input alone.  A list that breaks the
// ordering contract costs nothing but its values: successors always lie behind their entry, exits behind their block, and a store
// is made only below a block's own rank plus its own count.
#pragma once
#include "disjoint_launch.hpp"
#include "prefix_kernel.hpp"
#include "scan_filters.hpp"

namespace ss {

constexpr uint32_t kDjBlock = SS_DISJOINT_BLOCK;
constexpr int kDjPer = (int)(kDjBlock / kDisjointThreads);
constexpr uint16_t kDjEnd = (uint16_t)kDjBlock;                 // a successor beyond the block
static_assert(kDjBlock % kDisjointThreads == 0 && kDjBlock <= 32768 && (kDjBlock & (kDjBlock - 1)) == 0, "local indices are 16-bit");

// the first index k of [lo, hi) with a[k] >= t, else hi
template <class Index>
__device__ __forceinline__ Index dj_lower_bound(const uint64_t *a, Index lo, Index hi, uint64_t t)
{
    while (lo < hi) {
        const Index mid = lo + (hi - lo) / 2;
        if (a[mid] < t) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// the number of entries of a[lo, hi) at or below x, plus lo
__device__ __forceinline__ uint64_t dj_upper_bound(const uint64_t *a, uint64_t lo, uint64_t hi, uint64_t x)
{
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (a[mid] <= x) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ bool dj_is_head(uint64_t prev, uint64_t p, uint64_t n) { return p >= prev && p - prev >= n; }

// Stages the block's offsets, gives every entry its successor inside the block (kDjEnd: none) and finds the block's first head.
__device__ __forceinline__ void dj_stage(const DisjointArgs &a, uint64_t base, uint32_t len, uint64_t *s_off, uint16_t *s_succ, uint32_t *s_head)
{
    if (threadIdx.x == 0) *s_head = kDisjointNone;
    for (uint32_t j = threadIdx.x; j < len; j += kDisjointThreads) s_off[j] = a.offsets[base + j];
    __syncthreads();
    uint32_t first = kDisjointNone;
    for (uint32_t j = threadIdx.x; j < len; j += kDisjointThreads) {
        const uint64_t p = s_off[j];
        uint32_t succ = kDjEnd;
        if (p <= ~0ull - a.n) {
            const uint32_t hi = a.n < (uint64_t)(len - j) ? j + (uint32_t)a.n : len;
            const uint32_t k = dj_lower_bound<uint32_t>(s_off, j + 1, hi, p + a.n);
            if (k < len) succ = k;
        }
        s_succ[j] = (uint16_t)succ;
        const bool head = j != 0 ? dj_is_head(s_off[j - 1], p, a.n) : (base == 0 || dj_is_head(a.offsets[base - 1], p, a.n));
        if (head && first == kDisjointNone) first = j;
    }
    if (first != kDisjointNone) atomicMin(s_head, first);          // (LDS)
    __syncthreads();
}

// Pointer doubling.  In: s_ptr[j] = the successor of j.  Out: s_cnt[j] = the entries of the walk j, succ(j), ... inside the block
// and - kLast - s_last[j] = the last of them; every s_ptr[j] is kDjEnd.
template <bool kLast>
__device__ __forceinline__ void dj_double(uint32_t len, uint16_t *s_ptr, uint16_t *s_cnt, uint16_t *s_last)
{
    for (uint32_t j = threadIdx.x; j < len; j += kDisjointThreads) {
        s_cnt[j] = 1;
        if (kLast) s_last[j] = (uint16_t)j;
    }
    __syncthreads();
    for (uint32_t span = 1; span < kDjBlock; span <<= 1) {
        uint16_t np[kDjPer], nc[kDjPer], nl[kDjPer];
        int live = 0;
#pragma unroll
        for (int i = 0; i < kDjPer; ++i) {
            const uint32_t j = threadIdx.x + (uint32_t)i * kDisjointThreads;
            np[i] = kDjEnd;
            nc[i] = nl[i] = 0;
            if (j < len) {
                const uint16_t p = s_ptr[j];
                if (p != kDjEnd) {
                    np[i] = s_ptr[p];
                    nc[i] = (uint16_t)(s_cnt[j] + s_cnt[p]);
                    if (kLast) nl[i] = s_last[p];
                    live |= 1 << i;
                }
            }
        }
        if (!__syncthreads_or(live)) break;                         // (workgroup-uniform)
#pragma unroll
        for (int i = 0; i < kDjPer; ++i) {
            const uint32_t j = threadIdx.x + (uint32_t)i * kDisjointThreads;
            if (live & (1 << i)) {
                s_ptr[j] = np[i];
                s_cnt[j] = nc[i];
                if (kLast) s_last[j] = nl[i];
            }
        }
        __syncthreads();
    }
}

__global__ void __launch_bounds__(kDisjointThreads) disjoint_block_kernel(DisjointArgs a)
{
    __shared__ uint64_t s_off[kDjBlock];
    __shared__ uint16_t s_ptr[kDjBlock], s_cnt[kDjBlock], s_last[kDjBlock];
    __shared__ uint32_t s_head;
    const uint64_t base = (uint64_t)blockIdx.x * kDjBlock;
    const uint32_t len = a.count - base < kDjBlock ? (uint32_t)(a.count - base) : kDjBlock;
    const uint64_t end = base + len;
    dj_stage(a, base, len, s_off, s_ptr, &s_head);
    // A terminal's successor lies behind the block: its index in the whole list takes the place of its offset in LDS.
    uint64_t exit[kDjPer];
    int terminal = 0;
#pragma unroll
    for (int i = 0; i < kDjPer; ++i) {
        const uint32_t j = threadIdx.x + (uint32_t)i * kDisjointThreads;
        exit[i] = a.count;
        if (j < len && s_ptr[j] == kDjEnd) {
            terminal |= 1 << i;
            const uint64_t p = s_off[j], g = base + j;
            if (end < a.count && p <= ~0ull - a.n) {
                uint64_t hi = a.n < a.count - g ? g + a.n : a.count;
                if (hi < end) hi = end;
                exit[i] = dj_lower_bound<uint64_t>(a.offsets, end, hi, p + a.n);
            }
        }
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < kDjPer; ++i)
        if (terminal & (1 << i)) s_off[threadIdx.x + (uint32_t)i * kDisjointThreads] = exit[i];
    __syncthreads();
    dj_double<true>(len, s_ptr, s_cnt, s_last);
    const uint32_t head = s_head;
    if (threadIdx.x == 0) a.head[blockIdx.x] = head;
    for (uint32_t j = threadIdx.x; j < len; j += kDisjointThreads)
        if (head == kDisjointNone || j <= head)
            a.rec[base + j] = (uint64_t)s_cnt[j] << kDisjointExitBits | (s_off[s_last[j]] & kDisjointExitMask);
}

__global__ void __launch_bounds__(kDisjointThreads) disjoint_chain_kernel(DisjointArgs a)
{
    for (uint64_t b = threadIdx.x; b < a.blocks; b += kDisjointThreads) {
        a.entry[b] = b == 0 ? 0u : kDisjointNone;
        a.cnt[b] = 0;
    }
    __syncthreads();
    for (uint64_t b = threadIdx.x; b < a.blocks; b += kDisjointThreads) {
        const uint32_t head = a.head[b];
        if (head == kDisjointNone) continue;
        uint64_t e = a.rec[b * kDjBlock + head] & kDisjointExitMask;        // behind block b, whichever way it was entered
        while (e < a.count) {
            const uint64_t c = e / kDjBlock;
            const uint32_t at = (uint32_t)(e % kDjBlock), hc = a.head[c];
            if (hc != kDisjointNone) {
                a.entry[c] = at <= hc ? at : hc;                            // (at <= hc wherever the list ascends)
                break;
            }
            const uint64_t r = a.rec[e];
            a.entry[c] = at;
            a.cnt[c] = r >> kDisjointExitBits;
            e = r & kDisjointExitMask;                                      // behind block c
        }
    }
    __syncthreads();
    for (uint64_t b = threadIdx.x; b < a.blocks; b += kDisjointThreads) {
        const uint32_t head = a.head[b], at = a.entry[b];
        if (head != kDisjointNone && at != kDisjointNone) a.cnt[b] = a.rec[b * kDjBlock + at] >> kDisjointExitBits;
    }
}

__global__ void __launch_bounds__(kDisjointThreads) disjoint_emit_kernel(DisjointArgs a)
{
    __shared__ uint64_t s_off[kDjBlock];
    __shared__ uint16_t s_succ[kDjBlock], s_ptr[kDjBlock], s_cnt[kDjBlock];
    __shared__ uint32_t s_head;
    const uint32_t at = a.entry[blockIdx.x];
    const uint64_t rank = a.rank[blockIdx.x], want = a.cnt[blockIdx.x];
    if (at == kDisjointNone || want == 0 || rank >= a.capacity) return;    // (workgroup-uniform)
    const uint64_t base = (uint64_t)blockIdx.x * kDjBlock;
    const uint32_t len = a.count - base < kDjBlock ? (uint32_t)(a.count - base) : kDjBlock;
    dj_stage(a, base, len, s_off, s_succ, &s_head);
    for (uint32_t j = threadIdx.x; j < len; j += kDisjointThreads) s_ptr[j] = s_succ[j];
    __syncthreads();
    dj_double<false>(len, s_ptr, s_cnt, nullptr);
    const uint32_t from_entry = s_cnt[at];
    for (uint32_t j = threadIdx.x; j < len; j += kDisjointThreads) {
        if (j < at || (j != at && !dj_is_head(s_off[j - 1], s_off[j], a.n))) continue;
        uint32_t r = from_entry - s_cnt[j], k = j;                          // the entry and every head behind it are on its walk
        do {
            if (r >= want || rank + r >= a.capacity) break;
            a.out[rank + r] = s_off[k];
            ++r;
            k = s_succ[k];
        } while (k != kDjEnd && !dj_is_head(s_off[k - 1], s_off[k], a.n));
    }
}

__global__ void __launch_bounds__(kBlock) replace_kernel(ReplaceArgs a)
{
    __shared__ uint64_t s_slice[2];
    const uint64_t p0 = (uint64_t)blockIdx.x * SS_CONTEXT_PART_BYTES;
    const uint64_t p1 = p0 + SS_CONTEXT_PART_BYTES < a.hi ? p0 + SS_CONTEXT_PART_BYTES : a.hi;
    if (threadIdx.x < 2) {
        // the occurrences at or below the part's first byte - the last of them may have begun in a part before - and below its end
        const uint64_t q = threadIdx.x == 0 ? (p0 > a.lo ? p0 : a.lo) : p1 - 1;
        s_slice[threadIdx.x] = dj_upper_bound(a.sel, 0, a.nsel, q - a.lo);
    }
    __syncthreads();
    const uint64_t first = s_slice[0], last = s_slice[1];
    const uint64_t shift = a.rep_len - a.n;                                 // (modulo 2^64; out_len was checked on the host)
    for (uint64_t q0 = p0 + (uint64_t)threadIdx.x * 16; q0 < p1; q0 += (uint64_t)kBlock * 16) {
        if (q0 + 16 <= a.lo) continue;
        const uint4 v = *reinterpret_cast<const uint4 *>(a.base + q0);
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
        const uint64_t x0 = (q0 > a.lo ? q0 : a.lo) - a.lo;
        uint64_t idx = dj_upper_bound(a.sel, first, last, x0);              // occurrences at or below x0
        uint64_t cur = idx != 0 ? a.sel[idx - 1] : 0, nxt = idx < a.nsel ? a.sel[idx] : ~0ull;
#pragma unroll
        for (int t = 0; t < 16; ++t) {
            const uint64_t q = q0 + (uint64_t)t;
            if (q < a.lo || q >= a.hi) continue;
            const uint64_t x = q - a.lo;
            if (x == nxt) {
                ++idx;
                cur = nxt;
                nxt = idx < a.nsel ? a.sel[idx] : ~0ull;
            }
            if (idx != 0 && x - cur < a.n) {
                if (x == cur) {
                    uint8_t *dst = a.out + (cur + (idx - 1) * shift);
                    for (uint64_t k = 0; k < a.rep_len; ++k) dst[k] = a.rep[k];
                }
            } else {
                a.out[x + idx * shift] = (uint8_t)(w[t >> 2] >> ((t & 3) * 8));
            }
        }
    }
}

}  // namespace ss
