// batched_all_kernels.hpp - every occurrence for MANY (needle, haystack) problems in one grid (ss_count_batched /
// ss_find_all_batched, include/sliceslice_hip_matches_batched.h): the all-matches scan (scan_tiles<..., ALL = true>,
// scan_kernels.hpp) joined to the batched machinery (BatchDesc, BatchCold, plan_one, ColdInPlanT: batched_types.hpp; batch_cold_kernel of ss_batched.hip).
// Included by scan_inst_all_batched.hip only - libsliceslice_hip_matches_batched.so, none of the other libraries.
//
//   batch_all_plan_kernel     one lane per problem: the descriptor (plan_one, static byte classes), the initial count of a count
//                             call - 0, or len + 1 for the empty needle: no memset launch - and the empty needle's len + 1 where
//                             the scan grid finds it
//   batch_cold_kernel         (ss_batched.hip's, through launch_batch_cold) one lane per problem: the cold part ready-made, as plans have it.
//                             The all-matches mode is closed to LAZY_ORDER - no wave builds a schedule - so every problem gets one.
//   scan_all_batched_kernel   count x slices workgroups, PROBLEM-MAJOR (w = problem * slices + slice), slice s the CONTIGUOUS tiles
//                             [s * per, (s + 1) * per) of its problem: workgroup order is (problem, address) order, so the
//                             exclusive prefix sum of the workgroup counts is every workgroup's rank in the CSR output and the
//                             rows come out sorted with no sort.  One scalar load of the 64-byte descriptor, the hot Problem
//                             fields (pin_hot_fields, hot_problem: as scan_batched_plan_kernel), then the scan: no state word, no polls, no early
//                             exit, no PlanState.
//   prefix_kernel<uint64_t>   (prefix_kernel.hpp) exclusive prefix sum of the 64-bit workgroup counts, one workgroup
//   batch_rows_kernel         one lane per problem: d_row_begin and d_counts from the ranks
#pragma once
#include "scan_kernels.hpp"
#include "matches_batched_launch.hpp"        // (the modes: kBatchedAllCount / ...CountPerWorkgroup / ...Emit)
#include "batched_types.hpp"

namespace ss {

struct BatchedAllArgs {
    const BatchDesc *descs;
    const BatchCold *colds;
    const uint8_t *needles;
    uint64_t *counts;           // kBatchedAllCount: one per problem, initialised by the plan kernel (one add per workgroup with matches)
    uint64_t *wg_count;         // kBatchedAllCountPerWorkgroup: written, one per workgroup (zeros and surplus slices included); emit: read
    const uint64_t *wg_rank;    // kBatchedAllEmit: exclusive prefix sum of wg_count
    uint64_t *out;              // kBatchedAllEmit: the CSR offsets, ranks below capacity only
    uint64_t capacity;
    uint32_t nslices;
    uint32_t mode;
};

// A problem without a scan (BatchDesc::per == 0) that is an EMPTY NEEDLE carries its count, len + 1, in this field of its
// descriptor (plan_one leaves it zero there).
__device__ __forceinline__ uint64_t trivial_count(const BatchDesc &d) { return d.n == 0 ? d.nchunks_all : 0ull; }

// `counts` (may be null: find-all derives them from the ranks): the count call's output, complete for problems without a scan.
__global__ void __launch_bounds__(kBlock) batch_all_plan_kernel(const BatchArgs a, uint64_t count, BatchDesc *descs, uint32_t nslices,
                                                                 uint32_t min_tiles, uint64_t *counts)
{
    __shared__ uint8_t s_class[256];
    s_class[threadIdx.x] = (uint8_t)rarity_class4((uint8_t)threadIdx.x);        // the static classes: no sampling, no memory of earlier calls
    __syncthreads();
    const uint64_t prob = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (prob >= count) return;
    const uint64_t h0 = a.hay_begin[prob], h1 = a.hay_end[prob];
    const uint64_t n0 = a.needle_begin[prob], n1 = a.needle_end[prob];
    uint64_t tiles = 0;
    (void)plan_one(a, prob, h0, h1, n0, n1, 0, descs, nslices, min_tiles, kWavesPerBlock * 4, s_class, &tiles, false, nullptr);
    const uint64_t empty = n1 == n0 ? h1 - h0 + 1 : 0ull;                       // the empty needle matches at 0 .. len
    if (n1 == n0) descs[prob].nchunks_all = empty;
    if (counts) counts[prob] = empty;
}

// A lane counts in 32 bits (AllTiles::lane_count) and holds at most 31 matches per piece - its own 16 offsets and, with the exact
// compare, up to 15 flags handed over from the next lane - so at most 124 per tile (U = 4): the scan of a slice goes in runs of at
// most kAllRunTiles tiles (4 GiB of haystack), between which the lane's count moves into 64 bits.  (No test scans a slice of more
// than one run: that takes a single problem above 4 GiB in one workgroup.)
constexpr uint64_t kAllRunTiles = 1ull << 18;
static_assert(kAllRunTiles * 124 <= 0xffffffffull, "a lane's count of one run fits 32 bits");

__device__ __forceinline__ uint64_t wave_sum64(uint64_t v)
{
    // three limbs of 22 bits: each limb's sum over 64 lanes stays below 2^28
    const uint64_t l0 = wave_sum((uint32_t)v & 0x3FFFFFu), l1 = wave_sum((uint32_t)(v >> 22) & 0x3FFFFFu), l2 = wave_sum((uint32_t)(v >> 44));
    return l0 + (l1 << 22) + (l2 << 44);
}

template <bool EMIT>
__global__ void __launch_bounds__(kBlock) scan_all_batched_kernel(const BatchedAllArgs aa)
{
    __shared__ __attribute__((aligned(16))) uint8_t s_needle[kWavesPerBlock * kNeedleLds];
    __shared__ uint32_t s_wave[kWavesPerBlock];             // emit: the waves' counts of a tile (AllTiles::s_wave)
    __shared__ uint64_t s_sum[kWavesPerBlock];
    constexpr int U = 4;
    const uint32_t w = blockIdx.x;
    const uint32_t prob = w / aa.nslices, slice = w - prob * aa.nslices;
    const BatchDesc *dp = aa.descs + prob;
    BatchDesc d = *dp;
    pin_hot_fields(d);                              // in front of the kernel's first store
    const uint32_t eff = (uint32_t)(d.per >> 32), per = (uint32_t)d.per;
    constexpr bool emit = EMIT;
    uint64_t rank = 0;
    if (emit) {
        // only workgroups that hold one of the first `capacity` matches write (and re-read their tiles)
        const uint64_t cnt = uniform64(aa.wg_count[w]);
        rank = uniform64(aa.wg_rank[w]);
        if (cnt == 0 || rank >= aa.capacity) return;
    }
    if (slice >= eff) {                             // surplus slice, or a problem that needs no scan (eff == 0)
        const uint64_t mine = eff == 0 && slice == 0 ? trivial_count(d) : 0ull;
        if (aa.mode == kBatchedAllCountPerWorkgroup) {
            if (threadIdx.x == 0) aa.wg_count[w] = mine;
        } else if (emit) {
            // the empty needle's offsets 0 .. len at the problem's rank (only its slice-0 workgroup has a count)
            for (uint64_t i = threadIdx.x; i < mine && rank + i < aa.capacity; i += kBlock) aa.out[rank + i] = i;
        }
        return;                                     // (count calls: the plan kernel has answered)
    }
    const uint32_t mis = d.shifts & 15;
    const uint64_t npieces = ((mis + d.end + 15) / 16 + 63) / 64;
    const uint64_t ntiles = (npieces + kWavesPerBlock * U - 1) / (kWavesPerBlock * U);
    const uint64_t t0 = (uint64_t)slice * per;
    const uint64_t te = t0 + per < ntiles ? t0 + per : ntiles;
    Problem pr;                                     // hot fields only; the cold ones are re-read from the descriptor
    hot_problem(d, mis, npieces, pr);
    // the cold part ready-made by batch_cold_kernel, as plans have it; no state word, so no output pointer and no tally
    const ColdInPlanT<false> cold = {dp, aa.colds + prob, aa.needles, nullptr, nullptr};
    AllTiles at = {0u, emit, rank, aa.out, aa.capacity, s_wave};
    uint64_t mine = 0;
    for (uint64_t t = t0; t < te; t += kAllRunTiles) {
        const uint64_t tr = t + kAllRunTiles < te ? t + kAllRunTiles : te;
        at.lane_count = 0;
        // single stream, non-temporal loads; the second byte's window is run-time data (kQDynamic)
        if ((d.bytes >> 24) & 1) scan_tiles<0, 0, true, U, 1, false, false, false, ColdInPlanT<false>, true>(pr, cold, s_needle, t, 1, tr, &at);
        else scan_tiles<kQDynamic, 0, false, U, 1, false, false, false, ColdInPlanT<false>, true>(pr, cold, s_needle, t, 1, tr, &at);
        mine += at.lane_count;
    }
    if (emit) return;
    const uint64_t wc = wave_sum64(mine);
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    if (lane == 0) s_sum[wave] = wc;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint64_t sum = 0;
#pragma unroll
        for (int k = 0; k < kWavesPerBlock; ++k) sum += s_sum[k];
        if (aa.mode == kBatchedAllCountPerWorkgroup) aa.wg_count[w] = sum;
        else if (sum != 0) __hip_atomic_fetch_add(aa.counts + prob, sum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// One lane per problem (and one for the end): row_begin[p] = rank of the problem's first workgroup, row_begin[count] = the total,
// counts[p] (may be null) = the difference to the next row.
__global__ void __launch_bounds__(kBlock) batch_rows_kernel(const uint64_t *wg_rank, const uint64_t *total, uint64_t count, uint32_t nslices,
                                                             uint64_t *row_begin, uint64_t *counts)
{
    const uint64_t p = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (p > count) return;
    const uint64_t mine = p < count ? wg_rank[p * nslices] : *total;
    row_begin[p] = mine;
    if (counts && p < count) counts[p] = (p + 1 < count ? wg_rank[(p + 1) * nslices] : *total) - mine;
}

}  // namespace ss
