// runs_kernels.hpp - the kernels of the run calls (include/sliceslice_hip_runs.h has THE RULE; libsliceslice_hip_runs.so only:
// ss_runs.hip holds them and their host side).
//
//   runs_all_kernel<kRunsCount>                        ONE pass: every workgroup leaves its selected begins (and, where asked, ends) and
//                                                      adds the begins to the total
//   runs_all_kernel<kRunsEmit>                         the same grid again over the workgroups that hold one of the first `capacity`
//                                                      begins or ends: begin[k] = the k-th selected begin, end[k] = the k-th
//                                                      selected end + 1
//   runs_lines_kernel<kMaskedSum / kMaskedLineEmit>    one LineSum per workgroup / the records of the lines it closes
//
// Geometry, loads and view edges are masked_kernels.hpp's, called: masked_load<U>, set_valid_bits, kSetU, kSetTiles - 16 B per
// lane, 1 KiB per piece, 4 KiB per wave, 16 KiB per tile, 128 KiB per workgroup.
// MEMBERSHIP: a lane's 16-bit member mask of its 16 bytes, ANDed with the valid bits (absent bytes are non-members).  Range path
// (nranges != 0, wave-uniform): runs_in_range4 on the four dwords, one call per range.  Bitmap path: the 32-byte bitmap staged in
// LDS - eight dwords in eight banks, so equal bytes broadcast.  Line kernels clear the raw delimiter mask from the member mask.
// BEGINS AND ENDS: begins = m & ~((m << 1) | prev), ends = m & ~((m >> 1) | next << 15); prev = bit 15 of the lane in front, next =
// bit 0 of the lane behind: DPP inside a piece, readlane between a wave's pieces, one byte of memory at the wave's first and last
// byte, read only where that byte lies in the view.
// LENGTHS: with `simple` (wave-uniform) every begin and end is selected and nothing below runs.  Else a begin counts the members
// ahead of it in the 32-bit window (own mask | the next lane's << 16), an end those behind it in (the previous lane's | own << 16);
// a run that ends inside the window, or has reached `look` bytes there, is settled.  Only a run that reaches the window's edge
// undecided walks memory from that point, byte by byte against the bitmap in LDS, inside the view, at most up to `look` bytes.
// Runs are disjoint, so the walks' total work is linear in the view.
// COUNT / EMIT: per-lane counts, a wave sum, one word per workgroup for begins and one for ends, one add per workgroup to the
// total; ranks by wave_exclusive_sum as in masked_all_kernel<kMaskedEmit>.  No waiting between workgroups.
#pragma once
#include "masked_kernels.hpp"
#include "runs_launch.hpp"

namespace ss {

// lane l > 0 receives cur[l-1]; lane 0 keeps `first` (DPP wave_shr:1 without bound_ctrl)
__device__ __forceinline__ uint32_t from_prev_lane_or(uint32_t first, uint32_t cur)
{
    return (uint32_t)__builtin_amdgcn_update_dpp((int)first, (int)cur, 0x138 /* wave_shr:1 */, 0xf, 0xf, false);
}

__device__ __forceinline__ bool runs_member(const uint32_t *s_bits, uint32_t b) { return (s_bits[b >> 5] >> (b & 31u)) & 1u; }

// the member mask of a chunk, byte k at bit k
__device__ __forceinline__ uint32_t runs_members16(const RunsArgs &ra, const u32x4 &A, const uint32_t *s_bits)
{
    const uint32_t X[4] = {A.x, A.y, A.z, A.w};
    uint32_t m = 0;
    if (ra.nranges != 0) {                                                      // (wave-uniform)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            uint32_t z = runs_in_range4(X[j], ra.rg[0]);
            if (ra.nranges > 1) z |= runs_in_range4(X[j], ra.rg[1]);
            if (ra.nranges > 2) z |= runs_in_range4(X[j], ra.rg[2]);
            if (ra.nranges > 3) z |= runs_in_range4(X[j], ra.rg[3]);
            m |= masked_nibble(z) << (4 * j);
        }
    } else {
#pragma unroll
        for (int p = 0; p < 16; ++p) m |= (runs_member(s_bits, (X[p >> 2] >> (8 * (p & 3))) & 0xFFu) ? 1u : 0u) << p;
    }
    return m;
}

// the run that holds stream byte s - 1 and has L bytes up to there: its length as far as `look` needs it, walking ahead from s
__device__ __forceinline__ uint32_t runs_walk_ahead(const RunsArgs &ra, const uint32_t *s_bits, uint64_t s, uint32_t L)
{
    uint64_t i = s - ra.m.mis;                                                  // (s - 1 is a byte of the view)
    while (L < ra.look && i < ra.m.len && runs_member(s_bits, ra.m.hay[i])) {
        ++L;
        ++i;
    }
    return L;
}

// ... and the run that holds stream byte s + 1, walking back from s
__device__ __forceinline__ uint32_t runs_walk_back(const RunsArgs &ra, const uint32_t *s_bits, uint64_t s, uint32_t L)
{
    int64_t i = (int64_t)s - (int64_t)ra.m.mis;                                 // (-1: in front of the view)
    while (L < ra.look && i >= 0 && runs_member(s_bits, ra.m.hay[i])) {
        ++L;
        --i;
    }
    return L;
}

__device__ __forceinline__ bool runs_selected(const RunsArgs &ra, uint32_t L) { return L >= ra.min_len && (ra.max_len == 0 || L <= ra.max_len); }

// The selected begins (and, with ENDS, ends) of a wave's U pieces.  m[u] = the member masks (the line kernels have cleared the
// delimiters from them).
template <int U, bool ENDS>
__device__ __forceinline__ void runs_select(const RunsArgs &ra, const uint32_t *s_bits, uint64_t chunk0, int lane, uint32_t (&m)[U],
                                            uint32_t (&sb)[U], uint32_t (&se)[U])
{
    const MaskedArgs &a = ra.m;
    const uint64_t lo = a.mis, hi = a.mis + a.len;
    // the bytes in front of the wave's first and behind its last, where they are bytes of the view (wave-uniform)
    const uint64_t s0 = chunk0 * 16, s1 = (chunk0 + 64 * U) * 16;
    uint32_t pe = 0, ne = 0;
    if (s0 > lo && s0 <= hi) pe = runs_member(s_bits, a.base[s0 - 1]) ? 1u : 0u;
    if (s1 < hi) ne = runs_member(s_bits, a.base[s1]) ? 1u : 0u;
    uint32_t pm[U], nm[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const uint32_t first = u > 0 ? (uint32_t)__builtin_amdgcn_readlane((int)m[u - 1], kWave - 1) : pe << 15;
        const uint32_t last = u + 1 < U ? (uint32_t)__builtin_amdgcn_readlane((int)m[u + 1], 0) : ne;
        pm[u] = from_prev_lane_or(first, m[u]);
        nm[u] = from_next_lane_or(last, m[u]);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const uint32_t begins = m[u] & ~((m[u] << 1) | (pm[u] >> 15)) & 0xFFFFu;
        const uint32_t ends = m[u] & ~((m[u] >> 1) | ((nm[u] & 1u) << 15)) & 0xFFFFu;
        sb[u] = begins;
        se[u] = ENDS ? ends : 0u;
        if (ra.simple) continue;                                                // (wave-uniform)
        const uint64_t s = (chunk0 + 64 * u + (uint64_t)lane) * 16;             // the lane's first byte
        {
            // of the lane behind the wave's last one only bit 0 is known
            const uint32_t known = (u == U - 1 && lane == kWave - 1) ? 17u : 32u;
            const uint32_t w = m[u] | (nm[u] << 16);
            uint32_t c = begins, sel = 0;
            while (c != 0) {
                const uint32_t p = (uint32_t)__builtin_ctz(c);
                c &= c - 1;
                uint32_t L = (uint32_t)__builtin_ctzll(~(uint64_t)(w >> p));    // (<= known - p: the bits above are zero)
                if (L == known - p && L < ra.look) L = runs_walk_ahead(ra, s_bits, s + known, L);
                if (runs_selected(ra, L)) sel |= 1u << p;
            }
            sb[u] = sel;
        }
        if constexpr (ENDS) {
            // of the lane in front of the wave's first one only bit 15 is known
            const uint32_t known = (u == 0 && lane == 0) ? 1u : 16u;
            const uint32_t w = (pm[u] & 0xFFFFu) | (m[u] << 16);
            uint32_t c = ends, sel = 0;
            while (c != 0) {
                const uint32_t p = (uint32_t)__builtin_ctz(c);
                c &= c - 1;
                const uint32_t y = ~(w << (15u - p));                           // bit 31: the end itself
                uint32_t L = y == 0 ? 32u : (uint32_t)__builtin_clz(y);         // (<= p + 1 + known: the bits below are zero)
                if (L == p + 1 + known && L < ra.look) L = runs_walk_back(ra, s_bits, s - known - 1, L);
                if (runs_selected(ra, L)) sel |= 1u << p;
            }
            se[u] = sel;
        }
    }
}

// the member masks of a wave's U pieces; bytes outside the view are no members
template <int U>
__device__ __forceinline__ void runs_masks(const RunsArgs &ra, const u32x4 (&A)[U], const uint32_t *s_bits, uint64_t chunk0, int lane,
                                           uint32_t (&m)[U])
{
    const MaskedArgs &a = ra.m;
    const uint64_t lo = a.mis, hi = a.mis + a.len;
    const bool inner = chunk0 * 16 >= lo && (chunk0 + 64 * U) * 16 <= hi;       // (wave-uniform)
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const uint32_t ok = inner ? 0xFFFFu : set_valid_bits((chunk0 + 64 * u + lane) * 16, lo, hi);
        m[u] = runs_members16(ra, A[u], s_bits) & ok;
    }
}

template <int MODE>
__global__ void __launch_bounds__(kBlock) runs_all_kernel(RunsArgs ra)
{
    __shared__ uint32_t s_bits[8];
    __shared__ uint32_t s_wave[2 * kSetTiles * kWavesPerBlock];
    constexpr int U = kSetU;
    constexpr int wpb = kWavesPerBlock;
    const MaskedArgs &a = ra.m;
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
    const uint64_t t0 = (uint64_t)blockIdx.x * kSetTiles;
    const uint64_t t1 = t0 + kSetTiles < a.ntiles ? t0 + kSetTiles : a.ntiles;
    const bool ends = ra.wg_e != nullptr;                                       // (uniform)
    uint64_t run_b = 0, run_e = 0;                                              // emit: the index of the tile's first begin / end
    if constexpr (MODE == kRunsEmit) {
        run_b = uniform64(ra.rank_b[blockIdx.x]);
        run_e = uniform64(ra.rank_e[blockIdx.x]);
        const bool has_b = uniform64(ra.wg_b[blockIdx.x]) != 0 && run_b < a.capacity;
        const bool has_e = uniform64(ra.wg_e[blockIdx.x]) != 0 && run_e < a.capacity;
        if (!has_b && !has_e) return;                                           // (workgroup-uniform)
    }
    if (threadIdx.x < 8) s_bits[threadIdx.x] = ra.bits[threadIdx.x];
    __syncthreads();

    uint32_t lane_b = 0, lane_e = 0;
    for (uint64_t tile = t0; tile < t1; ++tile) {
        const uint64_t chunk0 = (tile * wpb + (uint64_t)wave) * (U * 64);
        u32x4 A[U];
        masked_load<U>(a, chunk0, lane, A);
        uint32_t m[U], sb[U], se[U];
        runs_masks<U>(ra, A, s_bits, chunk0, lane, m);
        if (MODE == kRunsEmit || ends) runs_select<U, true>(ra, s_bits, chunk0, lane, m, sb, se);
        else runs_select<U, false>(ra, s_bits, chunk0, lane, m, sb, se);
        uint32_t mine_b = 0, mine_e = 0;
#pragma unroll
        for (int u = 0; u < U; ++u) {
            mine_b += (uint32_t)__builtin_popcount(sb[u]);
            mine_e += (uint32_t)__builtin_popcount(se[u]);
        }
        if constexpr (MODE == kRunsCount) {
            lane_b += mine_b;
            lane_e += mine_e;
        } else {
            // the waves of this tile in address order
            const uint32_t tl = (uint32_t)(tile - t0);
            const uint32_t wb = wave_sum(mine_b), we = wave_sum(mine_e);
            if (lane == 0) {
                s_wave[2 * (tl * wpb + wave)] = wb;
                s_wave[2 * (tl * wpb + wave) + 1] = we;
            }
            __syncthreads();                                                    // (one slot per tile and wave: no slot is written twice)
            uint64_t base_b = run_b, base_e = run_e;
            for (int w = 0; w < wpb; ++w) {
                const uint32_t vb = s_wave[2 * (tl * wpb + w)], ve = s_wave[2 * (tl * wpb + w) + 1];
                if (w < wave) {
                    base_b += vb;
                    base_e += ve;
                }
                run_b += vb;
                run_e += ve;
            }
            const uint64_t g0 = chunk0 * 16 - a.mis;                            // hay index of the wave's first byte (mod 2^64)
            if (ra.out_b && wb != 0 && base_b < a.capacity) {                   // (wave-uniform)
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const uint32_t cnt = (uint32_t)__builtin_popcount(sb[u]);
                    uint64_t idx = base_b + wave_exclusive_sum(cnt, lane);
                    base_b += wave_sum(cnt);
                    uint32_t c = sb[u];
                    while (c != 0) {
                        const uint32_t p = (uint32_t)__builtin_ctz(c);
                        c &= c - 1;
                        if (idx < a.capacity) ra.out_b[idx] = g0 + (uint64_t)(64 * u + lane) * 16 + p;
                        ++idx;
                    }
                }
            }
            if (ra.out_e && we != 0 && base_e < a.capacity) {                   // (wave-uniform)
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const uint32_t cnt = (uint32_t)__builtin_popcount(se[u]);
                    uint64_t idx = base_e + wave_exclusive_sum(cnt, lane);
                    base_e += wave_sum(cnt);
                    uint32_t c = se[u];
                    while (c != 0) {
                        const uint32_t p = (uint32_t)__builtin_ctz(c);
                        c &= c - 1;
                        if (idx < a.capacity) ra.out_e[idx] = g0 + (uint64_t)(64 * u + lane) * 16 + p + 1;
                        ++idx;
                    }
                }
            }
            if (run_b >= a.capacity && run_e >= a.capacity) break;              // (workgroup-uniform: every wave has the same sums)
        }
    }
    if constexpr (MODE == kRunsCount) {
        const uint32_t wb = wave_sum(lane_b), we = wave_sum(lane_e);
        if (lane == 0) {
            s_wave[2 * wave] = wb;
            s_wave[2 * wave + 1] = we;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            uint64_t sum_b = 0, sum_e = 0;
            for (int w = 0; w < wpb; ++w) {
                sum_b += s_wave[2 * w];
                sum_e += s_wave[2 * w + 1];
            }
            if (ra.wg_b) ra.wg_b[blockIdx.x] = sum_b;
            if (ra.wg_e) ra.wg_e[blockIdx.x] = sum_e;
            if (a.total && sum_b != 0) (void)__hip_atomic_fetch_add(a.total, sum_b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

template <int MODE>
__global__ void __launch_bounds__(kBlock) runs_lines_kernel(RunsArgs ra)
{
    __shared__ uint32_t s_bits[8];
    __shared__ uint64_t s_last[kSetTiles * kMaxWavesPerBlock];
    __shared__ uint32_t s_flags[kSetTiles * kMaxWavesPerBlock];
    __shared__ uint32_t s_nd[kMaxWavesPerBlock], s_cl[kMaxWavesPerBlock];
    constexpr int U = kSetU;
    constexpr int wpb = kWavesPerBlock;
    const MaskedArgs &a = ra.m;
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
    if (threadIdx.x < 8) s_bits[threadIdx.x] = ra.bits[threadIdx.x];            // (the host has taken the delimiter out)
    __syncthreads();

    for (uint64_t tile = t0; tile < t1; ++tile) {
        const uint64_t chunk0 = (tile * wpb + (uint64_t)wave) * (U * 64);
        u32x4 A[U];
        masked_load<U>(a, chunk0, lane, A);
        uint32_t dmT[U], m[U], mk[U], se[U];
        line_capture<U>(A, chunk0, lane, lt, dmT);
        runs_masks<U>(ra, A, s_bits, chunk0, lane, m);
#pragma unroll
        for (int u = 0; u < U; ++u) m[u] &= ~line_ordered(dmT[u]);              // the delimiter is never a member
        runs_select<U, false>(ra, s_bits, chunk0, lane, m, mk, se);
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
