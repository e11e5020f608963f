// setmatches_kernels.hpp - the occurrence kernels of a needle set (include/sliceslice_hip_setmatches.h;
// libsliceslice_hip_setmatches.so only: ss_setmatches.hip holds them and their host side).
//
//   set_all_kernel<kSetAllCount>  ONE pass over the haystack for ALL needles of a set: every (offset, rank) pair adds 1 to its
//                                 needle's bin, and every workgroup leaves its number of pairs.
//   set_all_kernel<kSetAllEmit>   the same grid again; only the workgroups that hold one of the first `capacity` pairs read their
//                                 bytes again and write (offset, rank) at the pair's index.
//
// Geometry and lookup are set_scan_kernel's (needleset_kernels.hpp): the view from the aligned address below it, kSetTiles tiles per
// workgroup, kSetU pieces of 64 lanes x 16 bytes per wave and tile from non-temporal loads, both bitmaps staged in LDS and looked up
// with one LDS load per position, the byte behind a lane's last from the next lane (DPP), the next piece or memory.  There is no
// delimiter and no line: a position whose byte is in B1 or whose key is in B2 or P is a candidate, and EVERY candidate goes through
// set_each_at (needleset_tables.hpp, the text the host check runs), which walks the bucket to its end and reports each needle that
// occurs there in ascending rank.  An occurrence belongs to the lane that holds its first byte; the bytes behind it are read from
// memory, wherever they lie in the view.
//
// Count: a workgroup-private histogram of kSetHotSlots 32-bit bins in LDS (a workgroup covers 131,072 positions: no bin overflows)
// takes the needles that have a slot; a needle without one gets one relaxed 64-bit device-scope add per occurrence.  At the end
// every non-zero bin is flushed with one 64-bit add, and the workgroup's pairs go to one word or one add.  Integer adds commute, so
// the output is deterministic.
// Emit: address order is tile, wave, piece, lane, position, walk order.  Per tile every lane counts the pairs of its four pieces,
// the waves exchange their sums through LDS, and an exclusive prefix over the lanes ranks each piece's pairs; then the lane walks
// its candidates again and writes.  No sort.
#pragma once
#include "needleset_kernels.hpp"
#include "setmatches_launch.hpp"

namespace ss {

template <int MODE, bool FOLD>
__global__ void __launch_bounds__(kBlock) set_all_kernel(SetAllArgs a)
{
    __shared__ __attribute__((aligned(16))) uint32_t s_bp[kSetBpWords];
    __shared__ uint32_t s_b1[8];
    __shared__ uint32_t s_hist[MODE == kSetAllCount ? kSetHotSlots : 1];
    __shared__ uint32_t s_wave[kSetTiles * kWavesPerBlock];
    constexpr int U = kSetU;
    constexpr int wpb = kWavesPerBlock;
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
    const uint64_t t0 = (uint64_t)blockIdx.x * kSetTiles;
    const uint64_t t1 = t0 + kSetTiles < a.ntiles ? t0 + kSetTiles : a.ntiles;
    const uint64_t dlo = a.mis, dhi = a.mis + a.len;
    uint64_t run = 0;                                                           // emit: the index of the tile's first pair
    if constexpr (MODE == kSetAllEmit) {
        run = uniform64(a.wg_rank[blockIdx.x]);
        if (uniform64(a.wg[blockIdx.x]) == 0 || run >= a.capacity) return;      // (workgroup-uniform)
    }
    for (unsigned i = threadIdx.x; i < kSetBpWords / 4; i += kBlock)
        reinterpret_cast<u32x4 *>(s_bp)[i] = reinterpret_cast<const u32x4 *>(a.tv.bp)[i];
    if (threadIdx.x < 8) s_b1[threadIdx.x] = a.tv.b1[threadIdx.x];
    const bool bins = MODE == kSetAllCount && a.counts != nullptr;              // (uniform)
    if constexpr (MODE == kSetAllCount) {
        if (bins)
            for (unsigned i = threadIdx.x; i < kSetHotSlots; i += kBlock) s_hist[i] = 0;
    }
    __syncthreads();

    uint32_t lane_pairs = 0;                                                    // count: this lane's pairs
    for (uint64_t tile = t0; tile < t1; ++tile) {
        const uint64_t chunk0 = (tile * wpb + (uint64_t)wave) * (U * 64);
        const bool inner = chunk0 * 16 >= dlo && (chunk0 + 64 * U) * 16 <= dhi;  // (wave-uniform) every byte lies in the view
        u32x4 A[U];
        if (chunk0 + 64 * U <= a.nchunks) {
#pragma unroll
            for (int u = 0; u < U; ++u) A[u] = load_chunk<true>(a.base, chunk0 + 64 * u + lane);
        } else {
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const uint64_t c = chunk0 + 64 * u + lane;
                A[u] = u32x4{0, 0, 0, 0};
                if (c < a.nchunks) A[u] = load_chunk<true>(a.base, c);
            }
        }
        uint32_t ok0[U], cand[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if constexpr (FOLD) fold_ascii_chunk_keep(A[u], 0u);
            ok0[u] = inner ? 0xFFFFu : set_valid_bits((chunk0 + 64 * u + lane) * 16, dlo, dhi);
        }
        // the byte behind the wave's last one, from memory when it lies in the view
        uint32_t tail_x = 0, tail_ok = 0;
        {
            const uint64_t at = (chunk0 + 64 * U) * 16;
            if (at >= dlo && at < dhi) {
                tail_x = set_fold(a.base[at], FOLD ? 1u : 0u);
                tail_ok = 1u;
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const uint32_t last_x = u + 1 < U ? (uint32_t)__builtin_amdgcn_readlane((int)A[u + 1 < U ? u + 1 : u].x, 0) : tail_x;
            const uint32_t last_ok = u + 1 < U ? (uint32_t)__builtin_amdgcn_readlane((int)ok0[u + 1 < U ? u + 1 : u], 0) : tail_ok;
            const uint32_t D[5] = {A[u].x, A[u].y, A[u].z, A[u].w, from_next_lane_or(last_x, A[u].x)};
            const uint32_t ok17 = ok0[u] | (from_next_lane_or(last_ok, ok0[u]) & 1u) << 16;
            const uint32_t ok1 = ok0[u] & (ok17 >> 1);
            cand[u] = 0;
            if (__ballot(ok0[u] != 0) != 0) {                                   // (a piece outside the view: nothing to look up)
                uint32_t b2, pm;
                set_lookup16(s_bp, D, b2, pm);
                cand[u] = (b2 | pm) & ok1;
                if (a.tv.has1) cand[u] |= set_lookup16_b1(s_b1, D) & ok0[u];
            }
        }
        if constexpr (MODE == kSetAllCount) {
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const uint64_t g0 = (chunk0 + 64 * u + lane) * 16 - a.mis;        // hay index of the lane's byte 0 (wraps below the view:
                uint32_t c = cand[u];                                           //  no candidate lies there)
                while (c != 0) {
                    const uint32_t p = (uint32_t)__builtin_ctz(c);
                    c &= c - 1;
                    set_each_at(a.tv, a.tr, a.hay, a.len, g0 + p, a.how, [&](uint32_t rank) {
                        ++lane_pairs;
                        if (!bins) return;
                        const uint32_t s = a.tr.slot[rank];
                        if (s != kSetNoSlot) atomicAdd(&s_hist[s], 1u);
                        else (void)__hip_atomic_fetch_add(a.counts + rank, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    });
                }
            }
        } else {
            uint32_t cnt[U], mine = 0;
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const uint64_t g0 = (chunk0 + 64 * u + lane) * 16 - a.mis;
                uint32_t c = cand[u], n = 0;
                while (c != 0) {
                    const uint32_t p = (uint32_t)__builtin_ctz(c);
                    c &= c - 1;
                    set_each_at(a.tv, a.tr, a.hay, a.len, g0 + p, a.how, [&](uint32_t) { ++n; });
                }
                cnt[u] = n;
                mine += n;
            }
            // the waves of this tile in address order
            const uint32_t tl = (uint32_t)(tile - t0);
            const uint32_t wt = wave_sum(mine);
            if (lane == 0) s_wave[tl * wpb + wave] = wt;
            __syncthreads();                                                    // (one slot per tile and wave: no slot is written twice)
            uint64_t base = run;
            for (int w = 0; w < wpb; ++w) {
                const uint32_t v = s_wave[tl * wpb + w];
                if (w < wave) base += v;
                run += v;
            }
            if (wt != 0 && base < a.capacity) {                                 // (wave-uniform)
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    uint64_t idx = base + wave_exclusive_sum(cnt[u], lane);
                    base += wave_sum(cnt[u]);
                    const uint64_t g0 = (chunk0 + 64 * u + lane) * 16 - a.mis;
                    uint32_t c = cand[u];
                    while (c != 0) {
                        const uint32_t p = (uint32_t)__builtin_ctz(c);
                        c &= c - 1;
                        const uint64_t g = g0 + p;
                        set_each_at(a.tv, a.tr, a.hay, a.len, g, a.how, [&](uint32_t rank) {
                            if (idx < a.capacity) {
                                if (a.offsets) a.offsets[idx] = g;
                                if (a.ranks) a.ranks[idx] = rank;
                            }
                            ++idx;
                        });
                    }
                }
            }
            if (run >= a.capacity) break;                                       // (workgroup-uniform: every wave has the same `run`)
        }
    }
    if constexpr (MODE == kSetAllCount) {
        const uint32_t wt = wave_sum(lane_pairs);
        if (lane == 0) s_wave[wave] = wt;
        __syncthreads();                                                        // (also: every add to the bins has been made)
        if (bins) {
            for (unsigned s = threadIdx.x; s < a.tr.nhot; s += kBlock) {
                const uint32_t v = s_hist[s];
                if (v != 0) (void)__hip_atomic_fetch_add(a.counts + a.tr.hot[s], (uint64_t)v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
        if (threadIdx.x == 0) {
            uint64_t sum = 0;
            for (int w = 0; w < wpb; ++w) sum += s_wave[w];
            if (a.wg) a.wg[blockIdx.x] = sum;
            if (a.total && sum != 0) (void)__hip_atomic_fetch_add(a.total, sum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

}  // namespace ss
