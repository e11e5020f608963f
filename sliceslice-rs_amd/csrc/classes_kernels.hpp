// classes_kernels.hpp - the kernels of the byte-class calls (include/sliceslice_hip_classes.h has THE RULE;
// libsliceslice_hip_classes.so only: ss_classes.hip holds them and their host side).
//
//   classes_all_kernel<kMaskedCount / kMaskedEmit>        the occurrences: one word per workgroup and one add to the total / the offsets
//   classes_lines_kernel<kMaskedSum / kMaskedLineEmit>    one LineSum per workgroup / the records of the lines it closes
//
// Geometry, loads, filter, ownership, count, ranks, emit and the hand-over to line_capture / line_tile_done are masked_kernels.hpp's,
// called, on the COVER of every position (the tightest (value, mask) pair that accepts the position's set): masked_load and
// masked_filter on the two chosen positions give a superset of candidates in registers, masked_verify settles them against the
// covers staged in LDS.  New here is the EXACT TEST of what survives: the check list - one entry per position whose set is smaller
// than its cover, rarest set first - is walked from LDS; each entry reads hay[p + position] and tests its bit in the set's 32-byte
// bitmap in LDS; the walk leaves at the first miss.  Every lane of a wave walks the same list at its own step: lanes at one step
// read one dword (a broadcast), and the 8 dwords of a bitmap lie in 8 different banks, so lanes that test one set never conflict.
// A pattern without such positions has nchecks == 0 (wave-uniform) and returns what masked_all_kernel returns for its covers.
// Lines: a candidate that holds the delimiter is refused by masked_verify<true> whenever some SET accepts the delimiter
// (MaskedArgs::accepts); for every other pattern such a byte fails the compare or the exact test itself.
#pragma once
#include "classes_launch.hpp"
#include "masked_kernels.hpp"

namespace ss {

// bitmaps and check list: at most 512 + 1,024 dwords over 256 lanes
__device__ __forceinline__ void classes_stage(const ClassArgs &a, uint32_t *s_bits, uint32_t *s_chk)
{
    for (unsigned i = threadIdx.x; i < a.nbits; i += kBlock) s_bits[i] = a.ctab[i];
    for (unsigned i = threadIdx.x; i < a.nchecks; i += kBlock) s_chk[i] = a.ctab[a.nbits + i];
}

// hay[p + position] is in its set for every entry of the check list, h = the occurrence's first byte (all n bytes lie in the view)
__device__ __forceinline__ bool classes_exact(const uint8_t *h, const uint32_t *s_bits, const uint32_t *s_chk, uint32_t nchecks)
{
    for (uint32_t k = 0; k < nchecks; ++k) {
        const uint32_t e = s_chk[k];
        const uint32_t b = h[e & 0xFFFFu];
        if (((s_bits[(e >> 16) + (b >> 5)] >> (b & 31u)) & 1u) == 0) return false;
    }
    return true;
}

template <int MODE>
__global__ void __launch_bounds__(kBlock) classes_all_kernel(ClassArgs ca)
{
    __shared__ __attribute__((aligned(16))) uint32_t s_tab[2 * kMaskedMaxWords];
    __shared__ uint32_t s_bits[8 * kClassesMaxDistinct];
    __shared__ uint32_t s_chk[kClassesMaxInexact];
    __shared__ uint32_t s_wave[kSetTiles * kWavesPerBlock];
    constexpr int U = kSetU;
    constexpr int wpb = kWavesPerBlock;
    const MaskedArgs &a = ca.m;
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
    classes_stage(ca, s_bits, s_chk);
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
            const uint8_t *h0 = a.hay + ((chunk0 + 64 * u + lane) * 16 - a.mis - a.a);
            uint32_t c = hit[u];
            while (c != 0) {
                const uint32_t p = (uint32_t)__builtin_ctz(c);
                c &= c - 1;
                if (!masked_verify<false>(h0 + p, s_tab, a.n, 0u) || !classes_exact(h0 + p, s_bits, s_chk, ca.nchecks)) hit[u] &= ~(1u << p);
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
__global__ void __launch_bounds__(kBlock) classes_lines_kernel(ClassArgs ca)
{
    __shared__ __attribute__((aligned(16))) uint32_t s_tab[2 * kMaskedMaxWords];
    __shared__ uint32_t s_bits[8 * kClassesMaxDistinct];
    __shared__ uint32_t s_chk[kClassesMaxInexact];
    __shared__ uint64_t s_last[kSetTiles * kMaxWavesPerBlock];
    __shared__ uint32_t s_flags[kSetTiles * kMaxWavesPerBlock];
    __shared__ uint32_t s_nd[kMaxWavesPerBlock], s_cl[kMaxWavesPerBlock];
    constexpr int U = kSetU;
    constexpr int wpb = kWavesPerBlock;
    const MaskedArgs &a = ca.m;
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
    classes_stage(ca, s_bits, s_chk);
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
                    const bool cover = a.accepts ? masked_verify<true>(h0 + p, s_tab, a.n, dx4) : masked_verify<false>(h0 + p, s_tab, a.n, 0u);
                    if (cover && classes_exact(h0 + p, s_bits, s_chk, ca.nchecks)) mm |= 1u << p;
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
            // the wave summaries in address order, tile by tile and wave by wave, as masked_lines_kernel joins them
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
