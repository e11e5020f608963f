// context_kernels.hpp - the kernels of the context calls (include/sliceslice_hip_context.h; libsliceslice_hip_context.so only:
// ss_context.hip holds them and their host side).
//
//   context_census_kernel   the streaming pass: one workgroup per part of SS_CONTEXT_PART_BYTES counts the part's delimiter bytes from
//                           16-byte non-temporal loads - popcounts, a wave and a workgroup reduction, one 8-byte store.
//   prefix_kernel           (prefix_kernel.hpp) the delimiters in front of every part and in the whole view; later the output slots
//                           in front of every block of entries and the size of the output.
//   context_ranges_kernel   one thread per entry of the caller's numbers: how many lines it owns (context_ranges.hpp), scanned per
//                           block of kBlock entries.
//   context_fill_kernel     one thread per output slot below the capacity (grid-stride): the entry that owns it by a binary search
//                           in the slot prefix, then number and kind.
//   context_select_kernel   one workgroup per part.  Its first lane finds the entries whose lines can end or begin in the part; a
//                           part that holds no end and no beginning of an output line below the capacity leaves without loading a
//                           byte.  The others read their part again, give every delimiter its global rank r (lane prefix
//                           popcounts, wave offsets through LDS, the part's prefix) and look up lines r + 1 (it ends here) and
//                           r + 2 (it begins behind it) among those entries.
// The output numbers are never read back: fill and select both go from the caller's numbers and the slot prefix, so each of the
// four output arrays may be missing.  No global atomic; scratch is 16 bytes per part and 8 bytes and a little per entry.
#pragma once
#include "context_launch.hpp"
#include "context_ranges.hpp"
#include "prefix_kernel.hpp"
#include "scan_filters.hpp"

namespace ss {

constexpr uint64_t kCtxPartChunks = SS_CONTEXT_PART_BYTES / 16;                 // aligned 16-byte chunks of a part
constexpr int kCtxIters = (int)(kCtxPartChunks / kBlock);                       // ... per lane
constexpr uint64_t kCtxWaveChunks = kCtxPartChunks / kWavesPerBlock;            // ... per wave (select: a wave's chunks are contiguous)
constexpr uint64_t kCtxNone = ~0ull;
static_assert(kCtxPartChunks % kBlock == 0 && kCtxIters == 16, "a part is sixteen chunks per lane");

// bit k: byte k of the chunk equals the delimiter (dx4: the delimiter in every byte of a dword)
__device__ __forceinline__ uint32_t ctx_nibble(uint32_t f) { return ((f >> 7) & 1u) | ((f >> 14) & 2u) | ((f >> 21) & 4u) | ((f >> 28) & 8u); }
__device__ __forceinline__ uint32_t ctx_delim_bits(const u32x4 &A, uint32_t dx4)
{
    return ctx_nibble(zero_bytes_exact(A.x ^ dx4)) | ctx_nibble(zero_bytes_exact(A.y ^ dx4)) << 4 |
           ctx_nibble(zero_bytes_exact(A.z ^ dx4)) << 8 | ctx_nibble(zero_bytes_exact(A.w ^ dx4)) << 12;
}
// bit k: stream byte a0 + k lies in the view [lo, hi).  Preconditions: a0 < hi, and a0 + 16 > lo (lo < 16).
__device__ __forceinline__ uint32_t ctx_valid_bits(uint64_t a0, uint64_t lo, uint64_t hi)
{
    uint32_t vm = 0xFFFFu;
    if (a0 < lo) vm &= 0xFFFFu << (uint32_t)(lo - a0);
    if (a0 + 16 > hi) vm &= 0xFFFFu >> (uint32_t)(a0 + 16 - hi);
    return vm & 0xFFFFu;
}
__device__ __forceinline__ uint32_t ctx_wave_sum(uint32_t v)
{
    for (int d = kWave / 2; d > 0; d >>= 1) v += __shfl_xor(v, d, kWave);
    return v;
}
// N: the delimiters of the view, plus one when its last byte is none (hi > lo)
__device__ __forceinline__ uint64_t ctx_line_count(const CtxArgs &ca) { return *ca.ndelim + (ca.base[ca.hi - 1] != (uint8_t)ca.delim ? 1u : 0u); }

__global__ void __launch_bounds__(kBlock) context_census_kernel(CtxArgs ca)
{
    __shared__ uint32_t s_wave[kWavesPerBlock];
    const uint64_t c0 = (uint64_t)blockIdx.x * kCtxPartChunks, a0 = c0 * 16;
    const uint32_t dx4 = ca.delim * 0x01010101u;
    uint32_t n = 0;
    if (a0 >= ca.lo && a0 + SS_CONTEXT_PART_BYTES <= ca.hi) {                   // (workgroup-uniform) every byte of the part counts
        u32x4 A[kCtxIters];
#pragma unroll
        for (int i = 0; i < kCtxIters; ++i) A[i] = load_chunk<true>(ca.base, c0 + (uint64_t)i * kBlock + threadIdx.x);
#pragma unroll
        for (int i = 0; i < kCtxIters; ++i)
            n += __popc(zero_bytes_exact(A[i].x ^ dx4)) + __popc(zero_bytes_exact(A[i].y ^ dx4)) +
                 __popc(zero_bytes_exact(A[i].z ^ dx4)) + __popc(zero_bytes_exact(A[i].w ^ dx4));
    } else {                                                                    // the first and the last part: chunks that hold a byte of
        for (int i = 0; i < kCtxIters; ++i) {                                   // the view are loaded, the bytes outside it masked off
            const uint64_t c = c0 + (uint64_t)i * kBlock + threadIdx.x;
            if (c * 16 >= ca.hi) continue;
            const u32x4 A = load_chunk<true>(ca.base, c);
            n += __popc(ctx_delim_bits(A, dx4) & ctx_valid_bits(c * 16, ca.lo, ca.hi));
        }
    }
    n = ctx_wave_sum(n);
    if ((threadIdx.x & (kWave - 1)) == 0) s_wave[threadIdx.x / kWave] = n;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint64_t sum = 0;
        for (int w = 0; w < kWavesPerBlock; ++w) sum += s_wave[w];
        ca.cnt[blockIdx.x] = sum;
    }
}

// the lines entry e owns (e < count)
__device__ __forceinline__ CtxRange ctx_range_of(const CtxArgs &ca, uint64_t N, uint64_t e)
{
    const uint64_t prev = e > 0 ? ca.numbers[e - 1] : 0, next = e + 1 < ca.count ? ca.numbers[e + 1] : 0;
    return ctx_range(prev, ca.numbers[e], next, N, ca.before, ca.after);
}
// the first output slot of entry e
__device__ __forceinline__ uint64_t ctx_first_slot(const CtxArgs &ca, uint64_t e) { return ca.bpre[e / kBlock] + ca.first[e]; }

__global__ void __launch_bounds__(kBlock) context_ranges_kernel(CtxArgs ca)
{
    __shared__ uint64_t s_size[kBlock];
    const uint64_t e = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    const uint64_t size = e < ca.count ? ctx_size(ctx_range_of(ca, ctx_line_count(ca), e)) : 0;
    s_size[threadIdx.x] = size;
    __syncthreads();
    for (int d = 1; d < kBlock; d <<= 1) {                      // Hillis-Steele inclusive scan
        const uint64_t v = threadIdx.x >= (unsigned)d ? s_size[threadIdx.x - d] : 0ull;
        __syncthreads();
        s_size[threadIdx.x] += v;
        __syncthreads();
    }
    if (e < ca.count) ca.first[e] = s_size[threadIdx.x] - size;
    if (threadIdx.x == kBlock - 1) ca.bsum[blockIdx.x] = s_size[threadIdx.x];
}

// Slots ascend with the entries (the caller's contract); where they do not, every index below stays inside [0, count) and every
// write below the capacity, whatever the searches land on.
__global__ void __launch_bounds__(kBlock) context_fill_kernel(CtxArgs ca)
{
    const uint64_t total = *ca.total, n = total < ca.capacity ? total : ca.capacity;
    const uint64_t N = ctx_line_count(ca), blocks = (ca.count + kBlock - 1) / kBlock;
    for (uint64_t slot = (uint64_t)blockIdx.x * kBlock + threadIdx.x; slot < n; slot += (uint64_t)gridDim.x * kBlock) {
        uint64_t lo = 0, hi = blocks;                           // the last block whose first slot is <= slot ...
        while (lo < hi) {
            const uint64_t mid = lo + (hi - lo) / 2;
            if (ca.bpre[mid] <= slot) lo = mid + 1; else hi = mid;
        }
        const uint64_t blk = lo ? lo - 1 : 0, rest = slot - ca.bpre[blk];
        const uint64_t e0 = blk * kBlock, e1 = e0 + kBlock < ca.count ? e0 + kBlock : ca.count;
        lo = e0;                                                // ... and the last entry of it whose first slot is
        hi = e1;
        while (lo < hi) {
            const uint64_t mid = lo + (hi - lo) / 2;
            if (ca.first[mid] <= rest) lo = mid + 1; else hi = mid;
        }
        const uint64_t e = lo > e0 ? lo - 1 : e0;
        const uint64_t line = ctx_range_of(ca, N, e).lo + (rest - ca.first[e]);
        if (ca.out_number) ca.out_number[slot] = line;
        if (ca.out_kind) ca.out_kind[slot] = line == ca.numbers[e] ? 1 : 0;
    }
}

// the first index in [lo, hi) whose number is above `line` (hi: none)
__device__ __forceinline__ uint64_t ctx_upper(const uint64_t *numbers, uint64_t lo, uint64_t hi, uint64_t line)
{
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (numbers[mid] <= line) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// The output slot of line `line`, kCtxNone when it is no output line or its slot is not below the capacity.  [ea, eb]: entries
// outside them own no line near `line` (the workgroup's slice).  *more: the line behind it has the next slot.
__device__ __forceinline__ uint64_t ctx_slot_of(const CtxArgs &ca, uint64_t N, uint64_t ea, uint64_t eb, uint64_t line, bool *more)
{
    *more = false;
    const uint64_t at = ctx_upper(ca.numbers, ea, eb + 1, line);            // the selected line behind `line`; at - 1: the one at or in front of it
    for (int k = 0; k < 2; ++k) {
        if (k == 0 && at == 0) continue;
        const uint64_t e = k == 0 ? at - 1 : at;
        if (e >= ca.count) continue;
        const CtxRange r = ctx_range_of(ca, N, e);
        if (r.lo <= line && line <= r.hi) {
            const uint64_t slot = ctx_first_slot(ca, e) + (line - r.lo);
            if (slot >= ca.capacity) return kCtxNone;
            *more = line < r.hi && slot + 1 < ca.capacity;
            return slot;
        }
    }
    return kCtxNone;
}

__global__ void __launch_bounds__(kBlock) context_select_kernel(CtxArgs ca)
{
    __shared__ uint64_t s_slice[2];
    __shared__ uint32_t s_go, s_wave[kWavesPerBlock];
    const uint64_t pre = ca.pre[blockIdx.x], cnt = ca.cnt[blockIdx.x];
    const uint64_t N = ctx_line_count(ca);
    if (threadIdx.x == 0) {
        bool more;
        // the two records no delimiter writes: line 1 begins at 0, a last line without a delimiter ends at len
        if (blockIdx.x == 0 && ca.out_begin) {
            const uint64_t slot = ctx_slot_of(ca, N, 0, ca.count - 1, 1, &more);
            if (slot != kCtxNone) ca.out_begin[slot] = 0;
        }
        if (blockIdx.x == ca.parts - 1 && ca.out_end && N > *ca.ndelim) {
            const uint64_t slot = ctx_slot_of(ca, N, 0, ca.count - 1, N, &more);
            if (slot != kCtxNone) ca.out_end[slot] = ca.hi - ca.lo;
        }
        // lines pre + 1 .. pre + cnt end in this part, lines pre + 2 .. pre + cnt + 1 begin in it (the last one only if it exists)
        uint32_t go = 0;
        uint64_t ea = 0, eb = 0;
        if (cnt) {
            const uint64_t l0 = pre + 1, l1 = pre + cnt + 1 < N ? pre + cnt + 1 : N;
            eb = ctx_upper(ca.numbers, 0, ca.count, l1);                    // the first selected line behind the window ...
            if (eb == ca.count) eb = ca.count - 1;
            ea = ctx_upper(ca.numbers, 0, ca.count, l0 - 1);                // ... and the last one in front of it: their context may reach in
            if (ea > 0) --ea;
            if (ea > eb) ea = eb;
            go = 1;                                                         // (entries out of order: look, the lookups decide)
            for (uint64_t e = ea; e <= eb && e < ea + 4; ++e) {
                const CtxRange r = ctx_range_of(ca, N, e);
                const uint64_t x = r.lo > l0 ? r.lo : l0, y = r.hi < l1 ? r.hi : l1;
                if (r.lo <= r.hi && x <= y) {                               // the first wanted line of the part: slots ascend behind it
                    go = ctx_first_slot(ca, e) + (x - r.lo) < ca.capacity ? 1 : 0;
                    break;
                }
                if (e == eb) go = 0;                                        // no entry owns a line of the window
            }
        }
        s_go = go;
        s_slice[0] = ea;
        s_slice[1] = eb;
    }
    __syncthreads();
    if (!s_go) return;                                                      // (workgroup-uniform)
    const uint64_t ea = s_slice[0], eb = s_slice[1];
    const uint32_t dx4 = ca.delim * 0x01010101u, lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    const uint64_t c0 = (uint64_t)blockIdx.x * kCtxPartChunks + wave * kCtxWaveChunks + lane;
    uint32_t m[kCtxIters], mine = 0;
#pragma unroll
    for (int i = 0; i < kCtxIters; ++i) {
        const uint64_t c = c0 + (uint64_t)i * kWave;
        m[i] = 0;
        if (c * 16 < ca.hi) m[i] = ctx_delim_bits(load_chunk<true>(ca.base, c), dx4) & ctx_valid_bits(c * 16, ca.lo, ca.hi);
        mine += __popc(m[i]);
    }
    const uint32_t wsum = ctx_wave_sum(mine);
    if (lane == 0) s_wave[wave] = wsum;
    __syncthreads();
    uint64_t rank = pre;                                                    // delimiters of the view in front of this wave's chunks
    for (uint32_t w = 0; w < wave; ++w) rank += s_wave[w];
    const uint64_t below = lane ? ~0ull >> (kWave - lane) : 0ull;           // the lanes in front of this one
#pragma unroll
    for (int i = 0; i < kCtxIters; ++i) {
        const uint32_t c = __popc(m[i]);                                    // <= 16: five bit planes give the lanes' prefix
        uint32_t ex = 0, all = 0;
#pragma unroll
        for (int k = 0; k < 5; ++k) {
            const uint64_t bal = __ballot((c >> k) & 1u);
            ex += (uint32_t)__popcll(bal & below) << k;
            all += (uint32_t)__popcll(bal) << k;
        }
        uint64_t r = rank + ex;
        const uint64_t a0 = (c0 + (uint64_t)i * kWave) * 16;
        for (uint32_t bits = m[i]; bits; bits &= bits - 1, ++r) {
            const uint64_t pos = a0 + (uint32_t)__builtin_ctz(bits) - ca.lo;          // delimiter number r of the view: line r + 1 ends here
            bool more;
            const uint64_t slot = ctx_slot_of(ca, N, ea, eb, r + 1, &more);
            if (slot != kCtxNone && ca.out_end) ca.out_end[slot] = pos;
            if (!ca.out_begin || r + 2 > N) continue;                                  // line r + 2 begins behind it, if there is one
            const uint64_t next = more ? slot + 1 : ctx_slot_of(ca, N, ea, eb, r + 2, &more);
            if (next != kCtxNone) ca.out_begin[next] = pos + 1;
        }
        rank += all;
    }
}

}  // namespace ss
