// rewrite_kernels.hpp - the kernels of the rewrite call (include/sliceslice_hip_rewrite.h has THE RULE; libsliceslice_hip_rewrite.so
// only: ss_rewrite.hip holds them and their host side).
//
//   runs_replace_kernel<kRewriteSize>    ONE pass: every workgroup leaves its selected begins, its selected ends and
//                                        S = sum(e + 1) - sum(b) over them, in view coordinates, mod 2^64
//   runs_replace_kernel<kRewriteWrite>   the same grid again: every output byte put in place
//
// Geometry, loads, view edges, membership and begin / end selection are runs_kernels.hpp's, called: masked_load<U>, runs_masks<U>,
// runs_select<U, true> - 16 B per lane, 1 KiB per piece, 4 KiB per wave, 16 KiB per tile, 128 KiB per workgroup.
// SIZE: positions are counted from the workgroup's first stream byte (< 2^17), so a lane's sums fit 32 bits (at most 256 begins of
// 512 bytes) and so does a wave's; the workgroup's first lane moves them to view coordinates in 64 bits.
// INSIDE: x = begins ^ (ends << 1) has a bit wherever the state "inside a selected run" flips; its prefix-XOR over bits 0 .. 15 is
// the lane's inside mask, relative to the state at its first byte.  That state is the parity of the x bits in front of the lane:
// one ballot per piece and a count of the lanes below inside the wave; between waves and tiles through LDS, where every wave
// leaves (bytes kept if nothing is open at its first byte, bytes kept if a run is, begins, parity) and reads the waves in front
// of it behind ONE barrier per tile, as runs_all_kernel<kRunsEmit> does; in front of the workgroup from rank_b - rank_e.
// PLACE: a lane's output is popcount(keep) + popcount(begins) * rep_len bytes, keep = valid & ~inside; an exclusive sum over the
// lanes of a piece (skipped where every lane of the piece keeps all 16 bytes and begins nothing: the offsets are lane * 16), then
// pieces, waves and tiles in address order.
// STORE: a lane that keeps 16 bytes and begins nothing makes ONE unaligned 16-byte store; any other lane walks its kept bytes and
// begins in order, byte by byte, the text read from LDS; a text above kRewriteWaveText bytes is left out by the lane and copied by
// the whole wave, one begin at a time.  Every store is tested against out_len, so a haystack that changes between the passes
// cannot send one behind the output.  No waiting between workgroups.
#pragma once
#include "rewrite_launch.hpp"
#include "runs_kernels.hpp"

namespace ss {

typedef uint32_t rewrite_u32x4_unaligned __attribute__((ext_vector_type(4), aligned(1)));

// the sum of the positions of the set bits of a 16-bit mask
__device__ __forceinline__ uint32_t rewrite_position_sum(uint32_t m)
{
    return (uint32_t)(__builtin_popcount(m & 0xAAAAu) + 2 * __builtin_popcount(m & 0xCCCCu) + 4 * __builtin_popcount(m & 0xF0F0u) +
                      8 * __builtin_popcount(m & 0xFF00u));
}

// bit k = the XOR of bits 0 .. k, for k < 16
__device__ __forceinline__ uint32_t rewrite_prefix_xor(uint32_t x)
{
    x ^= x << 1;
    x ^= x << 2;
    x ^= x << 4;
    x ^= x << 8;
    return x & 0xFFFFu;
}

// byte p (0 .. 15) of a chunk, by selects: nothing is indexed at run time
__device__ __forceinline__ uint32_t rewrite_byte(const u32x4 &A, uint32_t p)
{
    const uint32_t lo = (p & 4u) ? A.y : A.x, hi = (p & 4u) ? A.w : A.z;
    return (((p & 8u) ? hi : lo) >> (8u * (p & 3u))) & 0xFFu;
}

template <int MODE>
__global__ void __launch_bounds__(kBlock) runs_replace_kernel(RewriteArgs wa)
{
    __shared__ uint32_t s_bits[8];
    __shared__ uint32_t s_wave[4 * kSetTiles * kWavesPerBlock];
    __shared__ uint32_t s_rep[MODE == kRewriteWrite ? kRewriteMaxText / 4 : 1];
    constexpr int U = kSetU;
    constexpr int wpb = kWavesPerBlock;
    const RunsArgs &ra = wa.r;
    const MaskedArgs &a = ra.m;
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
    const uint64_t t0 = (uint64_t)blockIdx.x * kSetTiles;
    const uint64_t t1 = t0 + kSetTiles < a.ntiles ? t0 + kSetTiles : a.ntiles;
    const uint32_t rep_len = wa.rep_len;
    const uint8_t *s_text = reinterpret_cast<const uint8_t *>(s_rep);
    uint64_t out_at = 0;                                                        // write: the output offset of the next tile's first byte
    uint32_t open = 0;                                                          // ... and whether a selected run is open there
    if constexpr (MODE == kRewriteWrite) {
        const uint64_t rank_b = uniform64(ra.rank_b[blockIdx.x]), rank_e = uniform64(ra.rank_e[blockIdx.x]);
        const uint64_t ps = uniform64(wa.rank_s[blockIdx.x]);
        const uint64_t P = blockIdx.x == 0 ? 0 : (uint64_t)blockIdx.x * kSetPartBytes - a.mis;    // view position of the first byte
        open = (uint32_t)(rank_b - rank_e) & 1u;
        out_at = P - (ps + (open ? P : 0)) + rank_b * rep_len;
        for (unsigned i = threadIdx.x; i < (rep_len + 3) / 4; i += kBlock) s_rep[i] = wa.rep[i];
    }
    if (threadIdx.x < 8) s_bits[threadIdx.x] = ra.bits[threadIdx.x];            // (the host has taken the delimiter out)
    __syncthreads();

    uint32_t lane_nb = 0, lane_ne = 0, lane_bs = 0, lane_es = 0;                // size
    for (uint64_t tile = t0; tile < t1; ++tile) {
        const uint64_t chunk0 = (tile * wpb + (uint64_t)wave) * (U * 64);
        const uint32_t tl = (uint32_t)(tile - t0);
        u32x4 A[U];
        masked_load<U>(a, chunk0, lane, A);
        uint32_t m[U], sb[U], se[U];
        runs_masks<U>(ra, A, s_bits, chunk0, lane, m);
        runs_select<U, true>(ra, s_bits, chunk0, lane, m, sb, se);
        if constexpr (MODE == kRewriteSize) {
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const uint32_t rel = ((tl * wpb + (uint32_t)wave) * (U * 64) + 64 * u + lane) * 16;     // from the workgroup's first byte
                const uint32_t cb = (uint32_t)__builtin_popcount(sb[u]), ce = (uint32_t)__builtin_popcount(se[u]);
                lane_nb += cb;
                lane_ne += ce;
                lane_bs += cb * rel + rewrite_position_sum(sb[u]);
                lane_es += ce * (rel + 1) + rewrite_position_sum(se[u]);
            }
        } else {
            const uint64_t lo = a.mis, hi = a.mis + a.len;
            const bool inner = chunk0 * 16 >= lo && (chunk0 + 64 * U) * 16 <= hi;                       // (wave-uniform)
            uint32_t valid[U], in[U];
            uint32_t carry = 0, c0 = 0, c1 = 0, nb = 0;
#pragma unroll
            for (int u = 0; u < U; ++u) {
                valid[u] = inner ? 0xFFFFu : set_valid_bits((chunk0 + 64 * u + lane) * 16, lo, hi);
                const uint32_t x = sb[u] ^ (se[u] << 1);
                const uint64_t flips = __builtin_amdgcn_ballot_w64((__builtin_popcount(x) & 1) != 0);
                const uint32_t below = __builtin_amdgcn_mbcnt_hi((uint32_t)(flips >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)flips, 0u));
                in[u] = rewrite_prefix_xor(x) ^ (((carry ^ below) & 1u) ? 0xFFFFu : 0u);
                carry ^= (uint32_t)__builtin_popcountll(flips) & 1u;
                c0 += (uint32_t)__builtin_popcount(valid[u] & ~in[u]);
                c1 += (uint32_t)__builtin_popcount(valid[u] & in[u]);
                nb += (uint32_t)__builtin_popcount(sb[u]);
            }
            // the waves of this tile in address order
            const uint32_t w0 = wave_sum(c0), w1 = wave_sum(c1), wb = wave_sum(nb);
            if (lane == 0) {
                uint32_t *slot = s_wave + 4 * (tl * wpb + wave);
                slot[0] = w0;
                slot[1] = w1;
                slot[2] = wb;
                slot[3] = carry;
            }
            __syncthreads();                                                    // (one slot per tile and wave: no slot is written twice)
            uint64_t at = 0;
            uint32_t mine = 0;
            for (int w = 0; w < wpb; ++w) {
                const uint32_t *slot = s_wave + 4 * (tl * wpb + w);
                const uint32_t v0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)slot[0]), v1 = (uint32_t)__builtin_amdgcn_readfirstlane((int)slot[1]);
                const uint32_t vb = (uint32_t)__builtin_amdgcn_readfirstlane((int)slot[2]), vp = (uint32_t)__builtin_amdgcn_readfirstlane((int)slot[3]);
                if (w == wave) {
                    at = out_at;
                    mine = open;
                }
                out_at += (uint64_t)(open ? v1 : v0) + (uint64_t)vb * rep_len;
                open ^= vp;
            }
            const uint32_t flip = mine ? 0xFFFFu : 0u;                          // (wave-uniform)
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const uint32_t keep = valid[u] & ~(in[u] ^ flip) & 0xFFFFu;
                const uint32_t beg = sb[u];
                const bool plain = keep == 0xFFFFu && beg == 0;
                uint64_t off;
                if (__builtin_amdgcn_ballot_w64(!plain) == 0) {                 // (wave-uniform) a piece that is copied whole
                    off = at + (uint64_t)lane * 16;
                    at += 64 * 16;
                } else {
                    const uint32_t size = (uint32_t)__builtin_popcount(keep) + (uint32_t)__builtin_popcount(beg) * rep_len;
                    off = at + wave_exclusive_sum(size, lane);
                    at += wave_sum(size);
                }
                if (plain) {
                    if (off + 16 <= wa.out_len) *reinterpret_cast<rewrite_u32x4_unaligned *>(wa.out + off) = A[u];
                } else {
                    uint64_t o = off;
                    uint32_t todo = keep | beg;
                    while (todo != 0) {
                        const uint32_t p = (uint32_t)__builtin_ctz(todo);
                        todo &= todo - 1;
                        if ((beg >> p) & 1u) {
                            if (rep_len <= kRewriteWaveText)
                                for (uint32_t i = 0; i < rep_len; ++i)
                                    if (o + i < wa.out_len) wa.out[o + i] = s_text[i];
                            o += rep_len;
                        } else {
                            if (o < wa.out_len) wa.out[o] = (uint8_t)rewrite_byte(A[u], p);
                            ++o;
                        }
                    }
                }
                if (rep_len > kRewriteWaveText) {                               // (wave-uniform) the texts of this piece, by the whole wave
                    uint64_t holders = __builtin_amdgcn_ballot_w64(beg != 0);
                    while (holders != 0) {
                        const int l = __builtin_ctzll(holders);
                        holders &= holders - 1;
                        uint32_t b = (uint32_t)__builtin_amdgcn_readlane((int)beg, l);
                        const uint32_t k = (uint32_t)__builtin_amdgcn_readlane((int)keep, l);
                        uint64_t dst = ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(off >> 32), l) << 32) |
                                       (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)off, l);
                        uint32_t kept = 0;                                      // the kept bytes of that lane in front of the begin
                        while (b != 0) {
                            const uint32_t p = (uint32_t)__builtin_ctz(b);
                            b &= b - 1;
                            const uint32_t now = (uint32_t)__builtin_popcount(k & ((1u << p) - 1u));
                            dst += now - kept;
                            kept = now;
                            for (uint32_t i = (uint32_t)lane; i < rep_len; i += kWave)
                                if (dst + i < wa.out_len) wa.out[dst + i] = s_text[i];
                            dst += rep_len;
                        }
                    }
                }
            }
        }
    }
    if constexpr (MODE == kRewriteSize) {
        const uint32_t wb = wave_sum(lane_nb), we = wave_sum(lane_ne), ws = wave_sum(lane_bs), wt = wave_sum(lane_es);
        if (lane == 0) {
            s_wave[4 * wave] = wb;
            s_wave[4 * wave + 1] = we;
            s_wave[4 * wave + 2] = ws;
            s_wave[4 * wave + 3] = wt;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            uint64_t nb = 0, ne = 0, bs = 0, es = 0;
            for (int w = 0; w < wpb; ++w) {
                nb += s_wave[4 * w];
                ne += s_wave[4 * w + 1];
                bs += s_wave[4 * w + 2];
                es += s_wave[4 * w + 3];
            }
            const uint64_t first = (uint64_t)blockIdx.x * kSetPartBytes - a.mis;       // view position of the first stream byte (mod 2^64)
            ra.wg_b[blockIdx.x] = nb;
            ra.wg_e[blockIdx.x] = ne;
            wa.wg_s[blockIdx.x] = es - bs + (ne - nb) * first;
        }
    }
}

}  // namespace ss
