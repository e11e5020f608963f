// needleset_kernels.hpp - the kernels of the needle-set calls (include/sliceslice_hip_needleset.h; libsliceslice_hip_needleset.so
// only: ss_needleset.hip holds them and their host side).
//
//   set_scan_kernel<kSetSum>      ONE pass over the haystack for ALL needles of a set (needleset_tables.hpp) that leaves one LineSum
//                                 per workgroup, for lines_chunk_kernel and lines_combine_kernel (lines_kernels.hpp).
//   set_scan_kernel<kSetEmit>     set_emit_kernel: the same grid again; only the workgroups that close one of the first `capacity`
//   set_scan_kernel<kSetEmitInv>  selected lines read their bytes again and write the records at their rank - the lines with a
//                                 match, or (Inv) those without one, from the model's states as lines_emit_inverted_kernel does.
//
// Geometry: the view starts at the 16-byte aligned address at or below its first byte (stream position a = hay index + mis);
// workgroups are in address order, kSetTiles tiles each; a tile is one run of U pieces (64 lanes x 16 bytes, non-temporal 16-byte
// loads) per wave.  Bytes outside [mis, mis + len) are masked out of delimiters, keys and occurrences, so there are no edge kernels.
// Per position p a lane forms the key (b[p], b[p + 1]) - b[p + 1] of its last byte from the next lane (DPP), of a piece's last lane
// from the next piece, of a wave's last lane from memory - and looks both bitmaps up with ONE LDS load (B2 and P are interleaved,
// 16 KiB staged once per workgroup).  B1 and B2 hits are matches; P hits walk their bucket in global memory (set_walk), lane by
// lane, and a candidate whose line is already known to match within the lane is skipped.  With a bound every hit goes through
// set_match_at.  The lane's match mask and delimiter mask go to line_tile_done (lines_tiles.hpp) as they are.
// No global atomic; scratch is one LineSum and one LinePre per workgroup.
#pragma once
#include "lines_launch.hpp"
#include "lines_tiles.hpp"
#include "needleset_launch.hpp"

namespace ss {

// bit k: stream byte a0 + k lies in [lo, hi)
__device__ __forceinline__ uint32_t set_valid_bits(uint64_t a0, uint64_t lo, uint64_t hi)
{
    const uint32_t l = lo > a0 ? (lo - a0 >= 16 ? 16u : (uint32_t)(lo - a0)) : 0u;
    const uint32_t h = hi > a0 ? (hi - a0 >= 16 ? 16u : (uint32_t)(hi - a0)) : 0u;
    return h > l ? ((1u << h) - 1u) & ~((1u << l) - 1u) : 0u;
}

// the 16 keys of a lane: D[0 .. 3] its chunk, D[4] the dword behind it (byte 0 only is used); both bitmaps in one LDS load each
__device__ __forceinline__ void set_lookup16(const uint32_t *s_bp, const uint32_t (&D)[5], uint32_t &b2, uint32_t &pm)
{
    b2 = pm = 0;
#pragma unroll
    for (int p = 0; p < 16; ++p) {
        const int j = p >> 2, t = p & 3;
        const uint32_t key = (t == 3 ? __builtin_amdgcn_alignbyte(D[j + 1], D[j], 3) : D[j] >> (8 * t)) & 0xFFFFu;
        const uint32_t bits = s_bp[key >> 4] >> (2 * (key & 15));
        b2 |= (bits & 1u) << p;
        pm |= ((bits >> 1) & 1u) << p;
    }
}
__device__ __forceinline__ uint32_t set_lookup16_b1(const uint32_t *s_b1, const uint32_t (&D)[5])
{
    uint32_t m = 0;
#pragma unroll
    for (int p = 0; p < 16; ++p) {
        const uint32_t b = (D[p >> 2] >> (8 * (p & 3))) & 0xFFu;
        m |= ((s_b1[b >> 5] >> (b & 31)) & 1u) << p;
    }
    return m;
}

// is there a match of `mm` on the line of position p, as far as the lane's 16 bytes show it (dm: its delimiters)?
__device__ __forceinline__ bool set_line_known(uint32_t mm, uint32_t dm, uint32_t p)
{
    const uint32_t below = (1u << p) - 1u, above = ~((2u << p) - 1u) & 0xFFFFu;
    const uint32_t lo = mm & below, hi = mm & above;
    if (lo != 0) {
        const uint32_t q = 31u - (uint32_t)__builtin_clz(lo);                   // the nearest match below: no delimiter in (q, p)?
        if ((dm & below & ~((2u << q) - 1u)) == 0) return true;
    }
    if (hi != 0) {
        const uint32_t q = (uint32_t)__builtin_ctz(hi);                         // the nearest match above: no delimiter in (p, q)?
        if ((dm & above & ((1u << q) - 1u)) == 0) return true;
    }
    return false;
}

template <int MODE, bool FOLD>
__global__ void __launch_bounds__(kBlock) set_scan_kernel(SetArgs sa)
{
    __shared__ __attribute__((aligned(16))) uint32_t s_bp[kSetBpWords];
    __shared__ uint32_t s_b1[8];
    __shared__ uint64_t s_last[kSetTiles * kMaxWavesPerBlock];
    __shared__ uint32_t s_flags[kSetTiles * kMaxWavesPerBlock];
    __shared__ uint32_t s_nd[kMaxWavesPerBlock], s_cl[kMaxWavesPerBlock];
    constexpr int U = kSetU;
    constexpr int wpb = kWavesPerBlock;
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
    const uint64_t t0 = (uint64_t)blockIdx.x * kSetTiles;
    const uint64_t t1 = t0 + kSetTiles < sa.ntiles ? t0 + kSetTiles : sa.ntiles;
    LineTiles lt;
    lt.delim_x4 = sa.delim * 0x01010101u;
    lt.dlo = sa.mis;
    lt.dhi = sa.mis + sa.len;
    lt.hshift = -(int64_t)sa.mis;
    lt.emit = MODE != kSetSum;
    lt.tile0 = t0;
    lt.lane_ndelim = lt.lane_closed = 0;
    lt.s_last = s_last;
    lt.s_flags = s_flags;
    lt.s_nd = s_nd;
    lt.s_cl = s_cl;
    lt.at = LinePre{0, 0, 0, 0, 0};
    lt.begin = sa.begin;
    lt.end = sa.end;
    lt.number = sa.number;
    lt.capacity = sa.capacity;
    if constexpr (MODE != kSetSum) {
        const LinePre *p = sa.pre + blockIdx.x;
        lt.at.ndelim = uniform64(p->ndelim);
        lt.at.rank = uniform64(p->rank);
        lt.at.last = uniform64(p->last);
        lt.at.carry = (uint32_t)__builtin_amdgcn_readfirstlane((int)p->carry);
        const uint32_t closes = (uint32_t)__builtin_amdgcn_readfirstlane((int)p->closes);
        if constexpr (MODE == kSetEmit) {
            if (closes == 0 || lt.at.rank >= sa.capacity) return;               // (workgroup-uniform)
        } else {
            lt.at.closes = 0;
            const uint64_t ndelim = uniform64(sa.sum[blockIdx.x].ndelim);
            if ((closes != 0xFFFFFFFFu && ndelim == closes) || lt.at.ndelim - lt.at.rank >= sa.capacity) return;
        }
    }
    // the two bitmaps: 1,024 16-byte loads over 256 lanes
    for (unsigned i = threadIdx.x; i < kSetBpWords / 4; i += kBlock)
        reinterpret_cast<u32x4 *>(s_bp)[i] = reinterpret_cast<const u32x4 *>(sa.tv.bp)[i];
    if (threadIdx.x < 8) s_b1[threadIdx.x] = sa.tv.b1[threadIdx.x];
    __syncthreads();

    const uint32_t dx4 = lt.delim_x4;
    const uint32_t keepx4 = FOLD && (uint8_t)(sa.delim - 'A') < 26 ? dx4 : 0u;
    const bool bound = (sa.how & (kSetWord | kSetLine)) != 0;
    for (uint64_t tile = t0; tile < t1; ++tile) {
        const uint64_t chunk0 = (tile * wpb + (uint64_t)wave) * (U * 64);
        const bool inner = chunk0 * 16 >= lt.dlo && (chunk0 + 64 * U) * 16 <= lt.dhi;   // (wave-uniform) every byte lies in the view
        u32x4 A[U];
        if (chunk0 + 64 * U <= sa.nchunks) {
#pragma unroll
            for (int u = 0; u < U; ++u) A[u] = load_chunk<true>(sa.base, chunk0 + 64 * u + lane);
        } else {
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const uint64_t c = chunk0 + 64 * u + lane;
                A[u] = u32x4{0, 0, 0, 0};
                if (c < sa.nchunks) A[u] = load_chunk<true>(sa.base, c);
            }
        }
        uint32_t dmT[U], mk[U], ok0[U];
        line_capture<U>(A, chunk0, lane, lt, dmT);
        // the folded bytes; alive = in the view and not the delimiter, raw or folded
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if constexpr (FOLD) fold_ascii_chunk_keep(A[u], keepx4);
            const uint32_t dead = FOLD ? line_ordered(delimiter_bits(A[u], dx4)) : line_ordered(dmT[u]);
            const uint32_t vm = inner ? 0xFFFFu : set_valid_bits((chunk0 + 64 * u + lane) * 16, lt.dlo, lt.dhi);
            // (without the fold the clipped delimiter mask misses dead bytes outside the view only, which vm takes out)
            ok0[u] = vm & ~dead;
        }
        // the byte behind the wave's last one, from memory when it lies in the view
        uint32_t tail_x = 0, tail_ok = 0;
        {
            const uint64_t a = (chunk0 + 64 * U) * 16;
            if (a >= lt.dlo && a < lt.dhi) {
                const uint8_t raw = sa.base[a];
                tail_x = set_fold(raw, FOLD ? 1u : 0u);
                tail_ok = (raw == sa.delim || tail_x == sa.delim) ? 0u : 1u;
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const uint32_t last_x = u + 1 < U ? (uint32_t)__builtin_amdgcn_readlane((int)A[u + 1 < U ? u + 1 : u].x, 0) : tail_x;
            const uint32_t last_ok = u + 1 < U ? (uint32_t)__builtin_amdgcn_readlane((int)ok0[u + 1 < U ? u + 1 : u], 0) : tail_ok;
            const uint32_t D[5] = {A[u].x, A[u].y, A[u].z, A[u].w, from_next_lane_or(last_x, A[u].x)};
            const uint32_t ok17 = ok0[u] | (from_next_lane_or(last_ok, ok0[u]) & 1u) << 16;
            const uint32_t ok1 = ok0[u] & (ok17 >> 1);
            uint32_t mm = 0, cand = 0;
            if (__ballot(ok0[u] != 0) != 0) {                                   // (a piece outside the view: nothing to look up)
                uint32_t b2, pm;
                set_lookup16(s_bp, D, b2, pm);
                mm = b2 & ok1;
                cand = pm & ok1;
                if (sa.tv.has1) mm |= set_lookup16_b1(s_b1, D) & ok0[u];
                if (bound) {
                    cand |= mm;
                    mm = 0;
                }
            }
            if (cand != 0) {
                const uint32_t dm = line_ordered(dmT[u]);
                const uint64_t g0 = (chunk0 + 64 * u + lane) * 16 - sa.mis;       // hay index of the lane's byte 0 (wraps below the view:
                do {                                                            //  no candidate lies there)
                    const uint32_t p = (uint32_t)__builtin_ctz(cand);
                    cand &= cand - 1;
                    if (set_line_known(mm, dm, p)) continue;
                    const uint64_t g = g0 + p;
                    bool hit;
                    if (bound) {
                        hit = set_match_at(sa.tv, sa.hay, sa.len, g, sa.delim, sa.how);
                    } else {
                        // (the key again, from memory: indexing D by p would put the lane's bytes into scratch)
                        const uint32_t key = set_fold(sa.hay[g], FOLD ? 1u : 0u) | (uint32_t)set_fold(sa.hay[g + 1], FOLD ? 1u : 0u) << 8;
                        hit = set_walk(sa.tv, sa.hay, sa.len, g, key, sa.delim, 0);
                    }
                    if (hit) mm |= 1u << p;
                } while (cand != 0);
            }
            mk[u] = mm;
        }
        line_tile_done<U, MODE == kSetEmitInv>(lt, dmT, mk, tile, chunk0, lane, wave, wpb);
    }
    if constexpr (MODE == kSetSum) {
        const uint32_t wn = wave_sum(lt.lane_ndelim), wc = wave_sum(lt.lane_closed);
        if (lane == 0) {
            s_nd[wave] = wn;
            s_cl[wave] = wc;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            // the wave summaries in address order, tile by tile and wave by wave, as lines_scan_kernel joins them
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
                    if (e & kLineHead) ++firsts;                                // (counted by the wave; decided here)
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
            sa.sum[blockIdx.x] = sum;
        }
    }
}

}  // namespace ss
