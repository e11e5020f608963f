// masked_kernels.hpp - the kernels of the masked-pattern calls (include/sliceslice_hip_masked.h has THE RULE;
// libsliceslice_hip_masked.so only: ss_masked.hip holds them and their host side).
//
//   masked_all_kernel<kMaskedCount>       ONE pass over the haystack: every workgroup leaves its number of occurrences and adds it
//                                         to the total.
//   masked_all_kernel<kMaskedEmit>        the same grid again; only the workgroups that hold one of the first `capacity` occurrences
//                                         read their bytes again and write the offsets at their ranks.
//   masked_lines_kernel<kMaskedSum>       ONE pass that leaves one LineSum per workgroup for lines_chunk_kernel / lines_combine_kernel.
//   masked_lines_kernel<kMaskedLineEmit>  the same grid again over the workgroups that close one of the first `capacity` lines.
//
// Geometry is set_all_kernel's, unchanged: the view from the 16-byte aligned address at or below it, kSetTiles tiles per workgroup,
// kSetU pieces of 64 lanes x 16 bytes per wave and tile from non-temporal 16-byte loads, no edge kernels.
// Filter: stream position q is a candidate when the byte there passes (v0, m0) - pattern position a - and the byte at q + d passes
// (v1, m1): ((x ^ v0x4) & m0x4) | ((s ^ v1x4) & m1x4) has a zero byte there, x the lane's own registers and s the same registers
// moved down by the wave-uniform d <= 16 bytes.  The 16 bytes behind a lane come from the next lane (DPP), behind a piece from the
// next piece (readlane), behind the wave from memory where that chunk holds a byte of the view.  d is split into dwords (uniform
// selects between registers of constant index: nothing is indexed at run time) and bytes (v_alignbyte with a scalar shift).
// Ownership: the occurrence at q - a belongs to the lane that holds q, so address order is offset order; the valid q are exactly
// [mis + a, mis + len - n + a] - one set_valid_bits call - and for those both filter bytes and all n bytes lie in the view.
// Verify: masked dword compares of hay[p .. p + n) against the (value, mask) pairs staged once per workgroup in LDS; the last
// n % 4 bytes are read one by one, so no load leaves the view.  Line kernels whose pattern accepts the delimiter somewhere
// (MaskedArgs::accepts, wave-uniform) also refuse a candidate that holds the delimiter; for every other pattern a byte equal to
// the delimiter fails the compare itself.
// Count / emit / lines are set_all_kernel's and set_scan_kernel's: per-lane counts, a wave sum, one word and one add per
// workgroup; ranks by wave_exclusive_sum; match and raw delimiter masks to line_capture / line_tile_done.  No sort, no scratch per
// occurrence, no waiting between workgroups.
#pragma once
#include "masked_launch.hpp"
#include "needleset_kernels.hpp"

namespace ss {

// bits 7, 15, 23, 31 of z -> bits 0 .. 3
__device__ __forceinline__ uint32_t masked_nibble(uint32_t z) { return ((((z >> 7) & 0x01010101u) * 0x01020408u) >> 24) & 0xFu; }

// the U pieces of a wave's part of a tile; chunks behind the view read as zero
template <int U>
__device__ __forceinline__ void masked_load(const MaskedArgs &a, uint64_t chunk0, int lane, u32x4 (&A)[U])
{
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
}

// the filter's candidates of the U pieces: bit k of cand[u] = the lane's byte k of piece u is a valid q that passes both tests
template <int U>
__device__ __forceinline__ void masked_filter(const MaskedArgs &a, const u32x4 (&A)[U], uint64_t chunk0, int lane, uint32_t (&cand)[U])
{
    const uint64_t vlo = a.mis + a.a, vhi = a.mis + a.len - a.n + a.a + 1;       // the valid q
    const bool inner = chunk0 * 16 >= vlo && (chunk0 + 64 * U) * 16 <= vhi;      // (wave-uniform)
    const uint32_t dq = a.d >> 2, dr = a.d & 3u;                                 // (wave-uniform)
    u32x4 T = u32x4{0, 0, 0, 0};                                                 // the chunk behind the wave's last one
    if (a.d != 0 && chunk0 + 64 * U < a.nchunks) T = load_chunk<true>(a.base, chunk0 + 64 * U);
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const uint32_t ok = inner ? 0xFFFFu : set_valid_bits((chunk0 + 64 * u + lane) * 16, vlo, vhi);
        cand[u] = 0;
        if (__ballot(ok != 0) == 0) continue;                                   // (a piece without a valid q)
        const u32x4 &B = A[u + 1 < U ? u + 1 : u];
        const uint32_t lx = u + 1 < U ? (uint32_t)__builtin_amdgcn_readlane((int)B.x, 0) : T.x;
        const uint32_t ly = u + 1 < U ? (uint32_t)__builtin_amdgcn_readlane((int)B.y, 0) : T.y;
        const uint32_t lz = u + 1 < U ? (uint32_t)__builtin_amdgcn_readlane((int)B.z, 0) : T.z;
        const uint32_t lw = u + 1 < U ? (uint32_t)__builtin_amdgcn_readlane((int)B.w, 0) : T.w;
        uint32_t E[9] = {A[u].x, A[u].y, A[u].z, A[u].w, from_next_lane_or(lx, A[u].x), from_next_lane_or(ly, A[u].y),
                         from_next_lane_or(lz, A[u].z), from_next_lane_or(lw, A[u].w), 0u};
        if (dq & 4u) {
#pragma unroll
            for (int j = 0; j < 5; ++j) E[j] = E[j + 4];
        }
        if (dq & 2u) {
#pragma unroll
            for (int j = 0; j < 6; ++j) E[j] = E[j + 2];
        }
        if (dq & 1u) {
#pragma unroll
            for (int j = 0; j < 5; ++j) E[j] = E[j + 1];
        }
        const uint32_t X[4] = {A[u].x, A[u].y, A[u].z, A[u].w};
        uint32_t m16 = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint32_t s = __builtin_amdgcn_alignbyte(E[j + 1], E[j], dr);
            const uint32_t z = zero_bytes_exact(((X[j] ^ a.v0x4) & a.m0x4) | ((s ^ a.v1x4) & a.m1x4));
            m16 |= masked_nibble(z) << (4 * j);
        }
        cand[u] = m16 & ok;
    }
}

// (hay[i] & mask[i]) == value[i] for all i < n, h = the occurrence's first byte; DELIM: and no byte is the delimiter
template <bool DELIM>
__device__ __forceinline__ bool masked_verify(const uint8_t *h, const uint32_t *s_tab, uint32_t n, uint32_t dx4)
{
    const uint32_t full = n >> 2, rest = n & 3u;
    for (uint32_t k = 0; k < full; ++k) {
        const uint32_t x = reinterpret_cast<const UnalignedU32 *>(h + 4 * k)->v;
        const uint32_t v = s_tab[2 * k], m = s_tab[2 * k + 1];
        if ((x & m) != v) return false;
        if (DELIM && zero_bytes_exact(x ^ dx4) != 0) return false;
    }
    if (rest != 0) {
        const uint8_t *t = h + 4 * full;
        uint32_t x = t[0];
        if (rest > 1) x |= (uint32_t)t[1] << 8;
        if (rest > 2) x |= (uint32_t)t[2] << 16;
        const uint32_t v = s_tab[2 * full], m = s_tab[2 * full + 1];
        if ((x & m) != v) return false;
        if (DELIM && (zero_bytes_exact(x ^ dx4) & (0x00808080u >> (8 * (3 - rest)))) != 0) return false;
    }
    return true;
}

// the (value, mask) pairs: at most 2,048 dwords over 256 lanes
__device__ __forceinline__ void masked_stage(const MaskedArgs &a, uint32_t *s_tab)
{
    for (unsigned i = threadIdx.x; i < 2 * a.nw; i += kBlock) s_tab[i] = a.tab[i];
}

template <int MODE>
__global__ void __launch_bounds__(kBlock) masked_all_kernel(MaskedArgs a)
{
    __shared__ __attribute__((aligned(16))) uint32_t s_tab[2 * kMaskedMaxWords];
    __shared__ uint32_t s_wave[kSetTiles * kWavesPerBlock];
    constexpr int U = kSetU;
    constexpr int wpb = kWavesPerBlock;
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
    const uint64_t t0 = (uint64_t)blockIdx.x * kSetTiles;
    const uint64_t t1 = t0 + kSetTiles < a.ntiles ? t0 + kSetTiles : a.ntiles;
    uint64_t run = 0;                                                           // emit: the index of the tile's first occurrence
    if constexpr (MODE == kMaskedEmit) {
        run = uniform64(a.wg_rank[blockIdx.x]);
        if (uniform64(a.wg[blockIdx.x]) == 0 || run >= a.capacity) return;      // (workgroup-uniform)
    }
    masked_stage(a, s_tab);
    __syncthreads();

    uint32_t lane_hits = 0;                                                     // count: this lane's occurrences
    for (uint64_t tile = t0; tile < t1; ++tile) {
        const uint64_t chunk0 = (tile * wpb + (uint64_t)wave) * (U * 64);
        u32x4 A[U];
        masked_load<U>(a, chunk0, lane, A);
        uint32_t hit[U];
        masked_filter<U>(a, A, chunk0, lane, hit);
        uint32_t mine = 0;
#pragma unroll
        for (int u = 0; u < U; ++u) {
            // hay + the index of the occurrence whose q is the lane's byte 0 (below the view only where no candidate is)
            const uint8_t *h0 = a.hay + ((chunk0 + 64 * u + lane) * 16 - a.mis - a.a);
            uint32_t c = hit[u];
            while (c != 0) {
                const uint32_t p = (uint32_t)__builtin_ctz(c);
                c &= c - 1;
                if (!masked_verify<false>(h0 + p, s_tab, a.n, 0u)) hit[u] &= ~(1u << p);
            }
            mine += (uint32_t)__builtin_popcount(hit[u]);
        }
        if constexpr (MODE == kMaskedCount) {
            lane_hits += mine;
        } else {
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
                    const uint32_t cnt = (uint32_t)__builtin_popcount(hit[u]);
                    uint64_t idx = base + wave_exclusive_sum(cnt, lane);
                    base += wave_sum(cnt);
                    const uint64_t g0 = (chunk0 + 64 * u + lane) * 16 - a.mis - a.a;
                    uint32_t c = hit[u];
                    while (c != 0) {
                        const uint32_t p = (uint32_t)__builtin_ctz(c);
                        c &= c - 1;
                        if (idx < a.capacity) a.offsets[idx] = g0 + p;
                        ++idx;
                    }
                }
            }
            if (run >= a.capacity) break;                                       // (workgroup-uniform: every wave has the same `run`)
        }
    }
    if constexpr (MODE == kMaskedCount) {
        const uint32_t wt = wave_sum(lane_hits);
        if (lane == 0) s_wave[wave] = wt;
        __syncthreads();
        if (threadIdx.x == 0) {
            uint64_t sum = 0;
            for (int w = 0; w < wpb; ++w) sum += s_wave[w];
            if (a.wg) a.wg[blockIdx.x] = sum;
            if (a.total && sum != 0) (void)__hip_atomic_fetch_add(a.total, sum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

template <int MODE>
__global__ void __launch_bounds__(kBlock) masked_lines_kernel(MaskedArgs a)
{
    __shared__ __attribute__((aligned(16))) uint32_t s_tab[2 * kMaskedMaxWords];
    __shared__ uint64_t s_last[kSetTiles * kMaxWavesPerBlock];
    __shared__ uint32_t s_flags[kSetTiles * kMaxWavesPerBlock];
    __shared__ uint32_t s_nd[kMaxWavesPerBlock], s_cl[kMaxWavesPerBlock];
    constexpr int U = kSetU;
    constexpr int wpb = kWavesPerBlock;
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
    const uint64_t t0 = (uint64_t)blockIdx.x * kSetTiles;
    const uint64_t t1 = t0 + kSetTiles < a.ntiles ? t0 + kSetTiles : a.ntiles;
    LineTiles lt;
    lt.delim_x4 = a.delim * 0x01010101u;
    lt.dlo = a.mis;
    lt.dhi = a.mis + a.len;
    lt.hshift = -(int64_t)a.mis;
    lt.emit = MODE != kMaskedSum;
    lt.tile0 = t0;
    lt.lane_ndelim = lt.lane_closed = 0;
    lt.s_last = s_last;
    lt.s_flags = s_flags;
    lt.s_nd = s_nd;
    lt.s_cl = s_cl;
    lt.at = LinePre{0, 0, 0, 0, 0};
    lt.begin = a.begin;
    lt.end = a.end;
    lt.number = a.number;
    lt.capacity = a.capacity;
    if constexpr (MODE != kMaskedSum) {
        const LinePre *p = a.pre + blockIdx.x;
        lt.at.ndelim = uniform64(p->ndelim);
        lt.at.rank = uniform64(p->rank);
        lt.at.last = uniform64(p->last);
        lt.at.carry = (uint32_t)__builtin_amdgcn_readfirstlane((int)p->carry);
        const uint32_t closes = (uint32_t)__builtin_amdgcn_readfirstlane((int)p->closes);
        if (closes == 0 || lt.at.rank >= a.capacity) return;                    // (workgroup-uniform)
    }
    masked_stage(a, s_tab);
    __syncthreads();

    const uint32_t dx4 = lt.delim_x4;
    for (uint64_t tile = t0; tile < t1; ++tile) {
        const uint64_t chunk0 = (tile * wpb + (uint64_t)wave) * (U * 64);
        u32x4 A[U];
        masked_load<U>(a, chunk0, lane, A);
        uint32_t dmT[U], mk[U], cand[U];
        line_capture<U>(A, chunk0, lane, lt, dmT);
        masked_filter<U>(a, A, chunk0, lane, cand);
#pragma unroll
        for (int u = 0; u < U; ++u) {
            uint32_t mm = 0, c = cand[u];
            if (c != 0) {
                const uint32_t dm = line_ordered(dmT[u]);
                const uint8_t *h0 = a.hay + ((chunk0 + 64 * u + lane) * 16 - a.mis - a.a);
                do {
                    const uint32_t p = (uint32_t)__builtin_ctz(c);
                    c &= c - 1;
                    if ((dm >> p) & 1u) continue;                               // (the anchor byte is the delimiter)
                    if (set_line_known(mm, dm, p)) continue;
                    const bool hit = a.accepts ? masked_verify<true>(h0 + p, s_tab, a.n, dx4) : masked_verify<false>(h0 + p, s_tab, a.n, 0u);
                    if (hit) mm |= 1u << p;
                } while (c != 0);
            }
            mk[u] = mm;
        }
        line_tile_done<U, false>(lt, dmT, mk, tile, chunk0, lane, wave, wpb);
    }
    if constexpr (MODE == kMaskedSum) {
        const uint32_t wn = wave_sum(lt.lane_ndelim), wc = wave_sum(lt.lane_closed);
        if (lane == 0) {
            s_nd[wave] = wn;
            s_cl[wave] = wc;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            // the wave summaries in address order, tile by tile and wave by wave, as set_scan_kernel joins them
            LineSum sum = {0, 0, 0, 0, 0};
            for (int w = 0; w < wpb; ++w) {
                sum.ndelim += s_nd[w];
                sum.closed += s_cl[w];
            }
            uint32_t f = 0;
            uint64_t joins = 0, firsts = 0;
            for (uint64_t t = 0; t < t1 - t0; ++t) {
                for (int w = 0; w < wpb; ++w) {
                    const uint32_t slot = (uint32_t)t * kMaxWavesPerBlock + (uint32_t)w;
                    const uint32_t e = s_flags[slot];
                    if ((e & kLineHas) == 0) {
                        if (e & kLineHead) f |= (f & kLineHas) ? kLineTail : (kLineHead | kLineTail);
                        continue;
                    }
                    if (e & kLineHead) ++firsts;
                    if (f & kLineHas) {
                        if ((f & kLineTail) | (e & kLineHead)) ++joins;
                        f = kLineHas | (f & kLineHead) | (e & kLineTail);
                    } else {
                        f = kLineHas | ((f | e) & kLineHead) | (e & kLineTail);
                    }
                    sum.last = s_last[slot];
                }
            }
            sum.closed = sum.closed + joins - firsts;
            sum.flags = f;
            a.sum[blockIdx.x] = sum;
        }
    }
}

}  // namespace ss
