// anyof_kernels.hpp - the kernels of the union of ascending lists of line numbers (include/sliceslice_hip_anyof.h;
// libsliceslice_hip_anyof.so only: ss_anyof.hip holds them and their host side).
//
//   anyof_count_kernel   one workgroup per segment of SS_ANYOF_SEGMENT_LINES consecutive numbers.  Every lane finds, for one list at
//                        a time, the slice of the list that falls into the segment (two binary searches, anyof_segments.hpp); the
//                        waves then stride over the slices and set the numbers' bits in an 8 KiB bitmap in LDS (LDS atomic OR: a
//                        number that several lists hold sets its bit once).  After a barrier every lane counts the set bits of its
//                        eight words - or, for the complement, the clear ones, the last segment cut at `limit` - and the workgroup
//                        stores one 8-byte count.
//   prefix_kernel        (prefix_kernel.hpp) the output numbers in front of every segment, and the size of the output.
//   anyof_emit_kernel    a segment whose rank is at or above the capacity, or that holds nothing, leaves at once.  The others build
//                        the same bitmap again, scan the lanes' popcounts (wave shuffles, wave sums through LDS) and write their
//                        numbers ascending from the segment's rank, stopping at the capacity.
// No global atomic; the output depends on the lists alone, never on the order in which lanes run; scratch is 16 bytes per segment
// and the lists' offsets, nothing per line.
#pragma once
#include "anyof_launch.hpp"
#include "anyof_segments.hpp"
#include "prefix_kernel.hpp"
#include "scan_filters.hpp"

namespace ss {

using AnySeg = AnySegments<SS_ANYOF_SEGMENT_LINES>;
constexpr int kAnyWordsPerLane = (int)(AnySeg::kWords / kBlock);
static_assert(AnySeg::kWords == 2048 && AnySeg::kWords % kBlock == 0 && kAnyWordsPerLane == 8, "a bitmap is eight words per lane");

// The bitmap of segment g: bit set <=> some list holds the number.  Complete (and visible to every lane) on return.
__device__ __forceinline__ void any_build_bitmap(const AnyArgs &aa, uint64_t g, uint32_t *s_bits, uint64_t *s_lo, uint64_t *s_hi)
{
    for (uint32_t w = threadIdx.x; w < AnySeg::kWords; w += kBlock) s_bits[w] = 0;
    const uint64_t first = AnySeg::first(g), last = AnySeg::last(g, aa.limit);
    const uint32_t lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    for (uint32_t k0 = 0; k0 < aa.lists; k0 += kBlock) {                    // (workgroup-uniform) kBlock lists at a time
        __syncthreads();                                                    // the bitmap is clear; the slices of the round before are read
        AnySlice sl = {0, 0};
        if (k0 + threadIdx.x < aa.lists) {
            const uint64_t b = aa.off[k0 + threadIdx.x], e = aa.off[k0 + threadIdx.x + 1];
            if (b < e) sl = any_slice(aa.numbers, b, e, first, last);
        }
        s_lo[threadIdx.x] = sl.lo;
        s_hi[threadIdx.x] = sl.hi;
        __syncthreads();
        const uint32_t n = aa.lists - k0 < (uint32_t)kBlock ? aa.lists - k0 : (uint32_t)kBlock;
        for (uint32_t j = wave; j < n; j += kWavesPerBlock) {               // a wave per list, a lane per entry
            const uint64_t hi = s_hi[j];
            for (uint64_t i = s_lo[j] + lane; i < hi; i += kWave) {
                const uint64_t v = aa.numbers[i];
                if (any_inside(v, first, last)) atomicOr(&s_bits[AnySeg::word_of(v)], AnySeg::bit_of(v));
            }
        }
    }
    __syncthreads();
}

__global__ void __launch_bounds__(kBlock) anyof_count_kernel(AnyArgs aa)
{
    __shared__ uint32_t s_bits[AnySeg::kWords];
    __shared__ uint64_t s_lo[kBlock], s_hi[kBlock];
    __shared__ uint32_t s_wave[kWavesPerBlock];
    const uint64_t g = blockIdx.x;
    any_build_bitmap(aa, g, s_bits, s_lo, s_hi);
    const uint64_t valid = AnySeg::valid(g, aa.limit);
    uint32_t n = 0;
#pragma unroll
    for (int i = 0; i < kAnyWordsPerLane; ++i) {
        const uint32_t w = threadIdx.x * kAnyWordsPerLane + i;
        n += any_popc(AnySeg::out_bits(s_bits[w], w, valid, aa.complement));
    }
    for (int d = kWave / 2; d > 0; d >>= 1) n += __shfl_xor(n, d, kWave);
    if ((threadIdx.x & (kWave - 1)) == 0) s_wave[threadIdx.x / kWave] = n;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint64_t sum = 0;
        for (int w = 0; w < kWavesPerBlock; ++w) sum += s_wave[w];
        aa.cnt[g] = sum;
    }
}

__global__ void __launch_bounds__(kBlock) anyof_emit_kernel(AnyArgs aa)
{
    __shared__ uint32_t s_bits[AnySeg::kWords];
    __shared__ uint64_t s_lo[kBlock], s_hi[kBlock];
    __shared__ uint32_t s_wave[kWavesPerBlock];
    const uint64_t g = blockIdx.x, rank = aa.pre[g];
    if (rank >= aa.capacity || aa.cnt[g] == 0) return;                     // (workgroup-uniform)
    any_build_bitmap(aa, g, s_bits, s_lo, s_hi);
    const uint64_t valid = AnySeg::valid(g, aa.limit);
    const uint32_t lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    uint32_t bits[kAnyWordsPerLane], mine = 0;
#pragma unroll
    for (int i = 0; i < kAnyWordsPerLane; ++i) {
        const uint32_t w = threadIdx.x * kAnyWordsPerLane + i;
        bits[i] = AnySeg::out_bits(s_bits[w], w, valid, aa.complement);
        mine += any_popc(bits[i]);
    }
    uint32_t incl = mine;                                                   // the lanes' inclusive prefix inside the wave
    for (int d = 1; d < kWave; d <<= 1) {
        const uint32_t v = __shfl_up(incl, d, kWave);
        if (lane >= (uint32_t)d) incl += v;
    }
    if (lane == kWave - 1) s_wave[wave] = incl;
    __syncthreads();
    uint64_t slot = rank + (incl - mine);
    for (uint32_t w = 0; w < wave; ++w) slot += s_wave[w];
#pragma unroll
    for (int i = 0; i < kAnyWordsPerLane; ++i) {
        if (slot >= aa.capacity) break;
        slot = any_emit_word(bits[i], AnySeg::number_at(g, threadIdx.x * kAnyWordsPerLane + i, 0), slot, aa.capacity, aa.out);
    }
}

}  // namespace ss
