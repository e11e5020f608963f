// fields_kernels.hpp - the kernels of the field calls (include/sliceslice_hip_fields.h has THE RULE; libsliceslice_hip_fields.so
// only: ss_fields.hip holds them and their host side).
//
//   fields_kernel<kFieldsSum>     ONE pass: every workgroup leaves one FieldsSum - its delimiters, the events of its head and of its
//                                 tail, and the record begins and ends of the lines that begin inside it
//   fields_carry_kernel           ONE workgroup walks the summaries in order, kFieldsCarryChunk at a time, and leaves one FieldsPre
//                                 per workgroup: carry-in, line base, ranks.  It does not read the haystack.
//   fields_kernel<kFieldsEmit>    the same grid again over the workgroups that hold one of the first `capacity` begins or ends
//
// Geometry, loads, view edges and membership are the run kernels', called: masked_load<U>, set_valid_bits, runs_members16 - 16 B
// per lane, 1 KiB per piece, 4 KiB per wave, 16 KiB per tile, 128 KiB per workgroup.
// MASKS: per lane and piece a delimiter mask, and the EVENT mask - EACH: the separators (the set without the delimiter); MERGE: the
// begins of the runs of field bytes (the set is the field bytes; begins and ends by runs_select<U, true> with one bit of each
// neighbour).  The view's end closes a last line without delimiter: one more terminator bit in the lane of the view's last byte.
// COUNT: c(p) = the events of p's line in front of p.  In the lane: a popcount below p's bit, restarted behind the lane's last
// delimiter below p (fields_lane walks the lane's segments; a lane without delimiter has one).  Across the lanes of a piece: ONE
// exclusive prefix sum of (events behind the lane's last delimiter | delimiters << 16), a ballot of the lanes that hold a delimiter
// and one bpermute for the sum at the nearest such lane below.  Across pieces: wave-uniform, by readlane.  Across waves and tiles:
// every wave leaves (delimiters, head events, tail events, has) in LDS and reads the waves in front of it behind ONE barrier per
// tile, as runs_replace_kernel does; the emit pass needs a second barrier per tile for the waves' record counts.
// MARKERS: every record begin and every record end is a bit of the byte that settles it - EACH: the separator in front of field
// `first` (begin = p + 1) and the separator that ends field `last` (end = p); MERGE: the begin of run `first` and the end of run
// `last` (end = p + 1); first == 1 in EACH: the line's first byte; a terminator: end = its position where the line is selected
// and has no field `last`, and with KEEP_SHORT begin = end = its position where it is not.  One begin and one end per record, in
// address order, so the k-th begin and the k-th end are record k.  Counts are compared in 32 bits: against (first, last) behind a
// delimiter of the workgroup, against (first, last) minus the 64-bit carry-in, saturated, in front of its first one (the HEAD).
// The sum pass leaves the head's markers out; the carry kernel adds them from carry-in, head events and head ends alone.
// Expected: 90 to 96 VGPRs (A[4] = 16, seven masks, three prefix words and four marker words per piece), no scratch, 0.9 KiB of LDS
// (the bitmap, four words per tile and wave, two counts per tile and wave); the carry kernel 66 VGPRs and 13 KiB of LDS (two
// buffers each of the pair scan and of the three sums).  No waiting between workgroups, no atomic.
#pragma once
#include "fields_launch.hpp"
#include "runs_kernels.hpp"

namespace ss {

// what a count is compared with: in the head relative to the carry-in, saturated (0xFFFFFFFF: nothing reaches it)
struct FieldsTh {
    uint32_t tb;            // c(p) of the begin's event
    uint32_t te;            // `last`: the end's byte has last - 1 field ends of its line in front of it
    uint32_t need;          // a terminator's count selects the line from here on ...
    uint32_t lastlim;       // ... and closes the record below this
};

__device__ __forceinline__ uint32_t fields_rel(uint64_t x, uint64_t cin)
{
    return x >= cin && x - cin <= 0x7FFFFFFFull ? (uint32_t)(x - cin) : 0xFFFFFFFFu;
}

__device__ __forceinline__ FieldsTh fields_thresholds(uint64_t first, uint64_t last, bool merge, uint64_t cin)
{
    FieldsTh t;
    t.tb = merge ? fields_rel(first - 1, cin) : (first >= 2 ? fields_rel(first - 2, cin) : 0xFFFFFFFFu);
    t.te = last == 0 ? 0xFFFFFFFFu : fields_rel(last, cin);
    const uint64_t need = merge ? first : first - 1;
    t.need = need <= cin ? 0u : fields_rel(need, cin);
    t.lastlim = last == 0 ? 0xFFFFFFFFu : (last <= cin ? 0u : fields_rel(last, cin));
    return t;
}

// the position of set bit j (from 0) of x, which has more than j
__device__ __forceinline__ uint32_t fields_select(uint32_t x, uint32_t j)
{
    for (; j != 0; --j) x &= x - 1;
    return (uint32_t)__builtin_ctz(x);
}

struct FieldsMarks {
    uint32_t bm, bp;        // record begins: the byte that settles one, and whether the begin is the position behind it
    uint32_t em, ep;        // record ends likewise
    uint32_t head_ends;     // MERGE: field ends in the workgroup's head
};

// One lane's 16 bytes, segment by segment: ev = events, ee = what ends a field (EACH: the separators again; MERGE: the field ends),
// dm = delimiters, vt = the view's end as a terminator behind that byte.  c = the count at the lane's first byte, open = a field
// is open there (MERGE: the ends in front are c - open), head = no delimiter of the workgroup lies in front of it.  bplus / eplus
// (0 or 1, uniform): a begin / an end is the position behind its byte.
__device__ __forceinline__ void fields_lane(uint32_t bplus, uint32_t eplus, bool keep, bool head_live, const FieldsTh &th_abs,
                                            const FieldsTh &th_head, uint32_t ev, uint32_t ee, uint32_t open, uint32_t dm, uint32_t vt,
                                            uint32_t c, bool head, FieldsMarks &k)
{
    uint32_t rem = dm | vt, lo = 0;
    for (;;) {
        const uint32_t p = rem != 0 ? (uint32_t)__builtin_ctz(rem) : 15u;       // the segment's last bit
        const uint32_t seg = ((2u << p) - 1u) & ~((1u << lo) - 1u);
        const uint32_t tb = head ? th_head.tb : th_abs.tb, te = head ? th_head.te : th_abs.te;
        const bool live = !head || head_live;
        const uint32_t evs = ev & seg, ees = ee & seg;
        const uint32_t n = (uint32_t)__builtin_popcount(evs), ne = (uint32_t)__builtin_popcount(ees);
        if (head) k.head_ends += ne;
        if (live) {
            if (tb >= c && tb - c < n) {
                const uint32_t b = fields_select(evs, tb - c);
                k.bm |= 1u << b;
                k.bp |= bplus << b;
            }
            if (te != 0xFFFFFFFFu && te + open >= c + 1 && te + open - c - 1 < ne) {    // (c - open ends lie in front of the segment)
                const uint32_t b = fields_select(ees, te + open - c - 1);
                k.em |= 1u << b;
                k.ep |= eplus << b;
            }
        }
        if (rem == 0) break;
        if (live) {
            const uint32_t T = c + n, isv = (vt >> p) & 1u;
            const bool sel = T >= (head ? th_head.need : th_abs.need);
            if (sel && T < (head ? th_head.lastlim : th_abs.lastlim)) {
                k.em |= 1u << p;
                k.ep |= isv << p;
            }
            if (!sel && keep) {
                k.bm |= 1u << p;
                k.bp |= isv << p;
                k.em |= 1u << p;
                k.ep |= isv << p;
            }
        }
        rem &= rem - 1;
        lo = p + 1;
        c = 0;
        open = 0;
        head = false;
        if (lo > 15) break;
    }
}

template <int MODE>
__global__ void __launch_bounds__(kBlock) fields_kernel(FieldsArgs fa)
{
    __shared__ uint32_t s_bits[8];
    __shared__ uint32_t s_wave[4 * kSetTiles * kWavesPerBlock];
    __shared__ uint32_t s_cnt[3 * kSetTiles * kWavesPerBlock];
    __shared__ uint32_t s_edge[2];
    constexpr int U = kSetU;
    constexpr int wpb = kWavesPerBlock;
    const RunsArgs &ra = fa.r;
    const MaskedArgs &a = ra.m;
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
    const uint64_t t0 = (uint64_t)blockIdx.x * kSetTiles;
    const uint64_t t1 = t0 + kSetTiles < a.ntiles ? t0 + kSetTiles : a.ntiles;
    const bool merge = fa.merge != 0, keep = fa.keep != 0;                      // (uniform)
    const bool starts = !merge && fa.first == 1;                                // EACH, first == 1: a record begins where its line does
    uint64_t cin = 0, line0 = 0, run_b = 0, run_e = 0;
    if constexpr (MODE == kFieldsEmit) {
        const FieldsPre *p = fa.pre + blockIdx.x;
        cin = uniform64(p->carry);
        line0 = uniform64(p->lines);
        run_b = uniform64(p->rank_b);
        run_e = uniform64(p->rank_e);
        const uint32_t nb = (uint32_t)__builtin_amdgcn_readfirstlane((int)p->nb), ne = (uint32_t)__builtin_amdgcn_readfirstlane((int)p->ne);
        const bool has_b = nb != 0 && run_b < a.capacity, has_e = ne != 0 && run_e < a.capacity;
        if (!has_b && !has_e) return;                                           // (workgroup-uniform)
    }
    const FieldsTh th_abs = fields_thresholds(fa.first, fa.last, merge, 0), th_head = fields_thresholds(fa.first, fa.last, merge, cin);
    if (threadIdx.x < 8) s_bits[threadIdx.x] = ra.bits[threadIdx.x];            // (the host has taken the delimiter out)
    if (threadIdx.x < 2) s_edge[threadIdx.x] = 0;
    __syncthreads();

    const uint32_t dx4 = fa.delim * 0x01010101u;
    const uint64_t lo = a.mis, hi = a.mis + a.len;
    // the workgroup in front of the current tile (uniform, the same in every wave): events since its last delimiter (or its first
    // byte), whether it has one, its delimiters, the events of its head
    uint32_t wg_c = 0, wg_nd = 0, wg_he = 0;
    bool wg_has = false;
    uint32_t lane_b = 0, lane_e = 0, lane_hn = 0;                               // sum
    for (uint64_t tile = t0; tile < t1; ++tile) {
        const uint64_t chunk0 = (tile * wpb + (uint64_t)wave) * (U * 64);
        const uint32_t tl = (uint32_t)(tile - t0);
        u32x4 A[U];
        masked_load<U>(a, chunk0, lane, A);
        const bool inner = chunk0 * 16 >= lo && (chunk0 + 64 * U) * 16 <= hi;   // (wave-uniform)
        uint32_t ok[U], dm[U], m[U], ev[U], fe[U], vt[U], st[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const uint64_t s = (chunk0 + 64 * u + (uint64_t)lane) * 16;         // the lane's first byte
            ok[u] = inner ? 0xFFFFu : set_valid_bits(s, lo, hi);
            dm[u] = (masked_nibble(zero_bytes_exact(A[u].x ^ dx4)) | masked_nibble(zero_bytes_exact(A[u].y ^ dx4)) << 4 |
                     masked_nibble(zero_bytes_exact(A[u].z ^ dx4)) << 8 | masked_nibble(zero_bytes_exact(A[u].w ^ dx4)) << 12) & ok[u];
            m[u] = runs_members16(ra, A[u], s_bits) & ok[u];
            vt[u] = 0;
            if (hi - 1 >= s && hi - 1 < s + 16 && ((dm[u] >> (uint32_t)(hi - 1 - s)) & 1u) == 0) vt[u] = 1u << (uint32_t)(hi - 1 - s);
            st[u] = 0;
        }
        if (merge) {                                                            // (uniform)
            runs_select<U, true>(ra, s_bits, chunk0, lane, m, ev, fe);
        } else {
#pragma unroll
            for (int u = 0; u < U; ++u) {
                ev[u] = m[u];
                fe[u] = 0;
            }
        }
        if (starts) {                                                           // (uniform)
            const uint64_t s0 = chunk0 * 16;
            uint32_t pd = 0;                                                    // the byte in front of the wave's first is a delimiter
            if (s0 > lo && s0 <= hi) pd = a.base[s0 - 1] == (uint8_t)fa.delim ? 1u : 0u;
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const uint64_t s = (chunk0 + 64 * u + (uint64_t)lane) * 16;
                const uint32_t first = u > 0 ? (uint32_t)__builtin_amdgcn_readlane((int)dm[u - 1], kWave - 1) : pd << 15;
                const uint32_t pm = from_prev_lane_or(first, dm[u]);
                st[u] = ((dm[u] << 1) | (pm >> 15)) & ok[u];
                if (lo >= s && lo < s + 16) st[u] |= 1u << (uint32_t)(lo - s);
            }
        }
        // the count at every lane's first byte, relative to the wave's first byte where no delimiter of the wave lies in front
        uint32_t cl[U], ndl[U];
        bool hb[U];
        uint32_t pc = 0, w_nd = 0, w_he = 0;
        bool phas = false;
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const uint32_t d = dm[u];
            const uint32_t all = (uint32_t)__builtin_popcount(ev[u]);
            const uint32_t tail = d != 0 ? (uint32_t)__builtin_popcount(ev[u] & ~((2u << (31 - __builtin_clz(d))) - 1u)) : all;
            const uint32_t hc = d != 0 ? (uint32_t)__builtin_popcount(ev[u] & ((1u << __builtin_ctz(d)) - 1u)) : all;
            const uint32_t v = tail | ((uint32_t)__builtin_popcount(d) << 16);
            const uint32_t P = wave_exclusive_sum(v, lane);
            const uint32_t tot = (uint32_t)__builtin_amdgcn_readlane((int)(P + v), kWave - 1);
            const uint64_t D = __builtin_amdgcn_ballot_w64(d != 0);
            const uint64_t below = D & ((1ull << lane) - 1ull);
            const int k = below != 0 ? 63 - __builtin_clzll(below) : 0;
            const uint32_t pk = (uint32_t)__shfl((int)P, k, kWave);
            if (below != 0) {
                cl[u] = (P & 0xFFFFu) - (pk & 0xFFFFu);
                hb[u] = true;
            } else {
                cl[u] = pc + (P & 0xFFFFu);
                hb[u] = phas;
            }
            ndl[u] = w_nd + (P >> 16);
            if (D != 0) {                                                       // (wave-uniform)
                const int kl = __builtin_amdgcn_readfirstlane(63 - __builtin_clzll(D)), kf = __builtin_amdgcn_readfirstlane(__builtin_ctzll(D));
                if (!phas) {
                    w_he = pc + ((uint32_t)__builtin_amdgcn_readlane((int)P, kf) & 0xFFFFu) + (uint32_t)__builtin_amdgcn_readlane((int)hc, kf);
                    phas = true;
                }
                pc = (tot & 0xFFFFu) - ((uint32_t)__builtin_amdgcn_readlane((int)P, kl) & 0xFFFFu);
            } else {
                pc += tot & 0xFFFFu;
            }
            w_nd += tot >> 16;
        }
        if (!phas) w_he = pc;
        if (lane == 0) {
            uint32_t *slot = s_wave + 4 * (tl * wpb + wave);
            slot[0] = w_nd;
            slot[1] = w_he;
            slot[2] = pc;
            slot[3] = phas ? 1u : 0u;
        }
        if constexpr (MODE == kFieldsSum) {
            if (merge && lane == 0 && wave == 0 && tl == 0) s_edge[0] = m[0] & 1u;
            if (merge && lane == kWave - 1 && wave == wpb - 1 && tl == kSetTiles - 1) s_edge[1] = (m[U - 1] >> 15) & 1u;
        }
        __syncthreads();                                                        // (one slot per tile and wave: no slot is written twice)
        uint32_t my_c = 0, my_nd = 0;
        bool my_has = false;
        for (int w = 0; w < wpb; ++w) {
            const uint32_t *slot = s_wave + 4 * (tl * wpb + w);
            const uint32_t snd = (uint32_t)__builtin_amdgcn_readfirstlane((int)slot[0]), she = (uint32_t)__builtin_amdgcn_readfirstlane((int)slot[1]);
            const uint32_t ste = (uint32_t)__builtin_amdgcn_readfirstlane((int)slot[2]), shas = (uint32_t)__builtin_amdgcn_readfirstlane((int)slot[3]);
            if (w == wave) {
                my_c = wg_c;
                my_nd = wg_nd;
                my_has = wg_has;
            }
            if (shas != 0) {
                if (!wg_has) {
                    wg_he = wg_c + she;
                    wg_has = true;
                }
                wg_c = ste;
            } else {
                wg_c += she;
            }
            wg_nd += snd;
        }
        FieldsMarks mk[U];
        uint32_t mine_b = 0, mine_e = 0;
#pragma unroll
        for (int u = 0; u < U; ++u) {
            mk[u] = FieldsMarks{st[u], 0, 0, 0, 0};
            const uint32_t open = merge ? m[u] & ~ev[u] & 1u : 0u;              // the lane's first byte goes on with a field
            fields_lane(merge ? 0u : 1u, merge ? 1u : 0u, keep, MODE == kFieldsEmit, th_abs, th_head, ev[u], merge ? fe[u] : ev[u], open, dm[u],
                        vt[u], hb[u] ? cl[u] : cl[u] + my_c, !hb[u] && !my_has, mk[u]);
            ndl[u] += my_nd;
            mine_b += (uint32_t)__builtin_popcount(mk[u].bm);
            mine_e += (uint32_t)__builtin_popcount(mk[u].em);
            lane_hn += mk[u].head_ends;
        }
        if constexpr (MODE == kFieldsSum) {
            lane_b += mine_b;
            lane_e += mine_e;
        } else {
            // the waves of this tile in address order
            const uint32_t wb = wave_sum(mine_b), we = wave_sum(mine_e);
            if (lane == 0) {
                s_cnt[2 * (tl * wpb + wave)] = wb;
                s_cnt[2 * (tl * wpb + wave) + 1] = we;
            }
            __syncthreads();
            uint64_t base_b = run_b, base_e = run_e;
            for (int w = 0; w < wpb; ++w) {
                const uint32_t vb = s_cnt[2 * (tl * wpb + w)], ve = s_cnt[2 * (tl * wpb + w) + 1];
                if (w < wave) {
                    base_b += vb;
                    base_e += ve;
                }
                run_b += vb;
                run_e += ve;
            }
            const uint64_t g0 = chunk0 * 16 - a.mis;                            // hay index of the wave's first byte (mod 2^64)
            const bool put_b = (fa.out_b || fa.out_n) && wb != 0 && base_b < a.capacity;
            const bool put_e = fa.out_e && we != 0 && base_e < a.capacity;
            if (put_b || put_e) {                                               // (wave-uniform)
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const uint32_t cnt = (uint32_t)__builtin_popcount(mk[u].bm) | ((uint32_t)__builtin_popcount(mk[u].em) << 16);
                    const uint32_t ex = wave_exclusive_sum(cnt, lane);
                    const uint32_t tot = (uint32_t)__builtin_amdgcn_readlane((int)(ex + cnt), kWave - 1);
                    uint64_t ib = base_b + (ex & 0xFFFFu), ie = base_e + (ex >> 16);
                    base_b += tot & 0xFFFFu;
                    base_e += tot >> 16;
                    const uint64_t pos = g0 + (uint64_t)(64 * u + lane) * 16;
                    uint32_t c = put_b ? mk[u].bm : 0u;
                    while (c != 0) {
                        const uint32_t p = (uint32_t)__builtin_ctz(c);
                        c &= c - 1;
                        if (ib < a.capacity) {
                            if (fa.out_b) fa.out_b[ib] = pos + p + ((mk[u].bp >> p) & 1u);
                            if (fa.out_n) fa.out_n[ib] = line0 + 1 + ndl[u] + (uint32_t)__builtin_popcount(dm[u] & ((1u << p) - 1u));
                        }
                        ++ib;
                    }
                    c = put_e ? mk[u].em : 0u;
                    while (c != 0) {
                        const uint32_t p = (uint32_t)__builtin_ctz(c);
                        c &= c - 1;
                        if (ie < a.capacity) fa.out_e[ie] = pos + p + ((mk[u].ep >> p) & 1u);
                        ++ie;
                    }
                }
            }
            if (run_b >= a.capacity && run_e >= a.capacity) break;              // (workgroup-uniform: every wave has the same sums)
        }
    }
    if constexpr (MODE == kFieldsSum) {
        const uint32_t wb = wave_sum(lane_b), we = wave_sum(lane_e), wn = wave_sum(lane_hn);
        if (lane == 0) {
            s_cnt[3 * wave] = wb;
            s_cnt[3 * wave + 1] = we;
            s_cnt[3 * wave + 2] = wn;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            FieldsSum s = {wg_nd, wg_has ? wg_he : wg_c, wg_c, 0, 0, 0, 0, 0};
            for (int w = 0; w < wpb; ++w) {
                s.begins += s_cnt[3 * w];
                s.ends += s_cnt[3 * w + 1];
                s.head_ends += s_cnt[3 * w + 2];
            }
            if (blockIdx.x == gridDim.x - 1 && a.hay[a.len - 1] != (uint8_t)fa.delim) s.flags |= kFieldsVirtual;
            if (s_edge[0]) s.flags |= kFieldsFirstIn;
            if (s_edge[1]) s.flags |= kFieldsLastIn;
            fa.sum[blockIdx.x] = s;
        }
    }
}

// The segmented carry over the workgroups' summaries: "a workgroup with a delimiter replaces the carry by its tail, one without
// adds its events", as an inclusive scan of (has, value) pairs per chunk of kFieldsCarryChunk summaries, then the record begins
// and ends of every workgroup - its own plus what its head line adds, which follows from carry-in, head events and head ends -
// as three plain sums.  Between chunks the state is four 64-bit words and one flag, the same in every lane.
__global__ void __launch_bounds__(kFieldsCarryChunk) fields_carry_kernel(FieldsCarryArgs ca)
{
    constexpr int C = kFieldsCarryChunk;
    __shared__ uint64_t s_val[2][C];
    __shared__ uint32_t s_has[2][C];
    __shared__ uint32_t s_nb[2][C], s_ne[2][C], s_nd[2][C];
    __shared__ uint32_t s_flags[C];
    const int i = (int)threadIdx.x;
    uint64_t carry = 0, lines = 0, rb = 0, re = 0;
    uint32_t prev_last = 0;
    for (uint64_t base = 0; base < ca.parts; base += C) {
        const uint64_t w = base + (uint64_t)i;
        FieldsSum s = {0, 0, 0, 0, 0, 0, 0, 0};                                 // (behind the last summary: passes the carry on)
        if (w < ca.parts) s = ca.sum[w];
        s_has[0][i] = s.nd != 0 ? 1u : 0u;
        s_val[0][i] = s.nd != 0 ? s.tail_events : s.head_events;
        s_flags[i] = s.flags;
        __syncthreads();
        int cur = 0;
        for (int d = 1; d < C; d <<= 1) {
            uint32_t h = s_has[cur][i];
            uint64_t v = s_val[cur][i];
            if (i >= d && h == 0) {
                h = s_has[cur][i - d];
                v += s_val[cur][i - d];
            }
            s_has[cur ^ 1][i] = h;
            s_val[cur ^ 1][i] = v;
            __syncthreads();
            cur ^= 1;
        }
        const uint32_t xh = i != 0 ? s_has[cur][i - 1] : 0u;
        const uint64_t xv = i != 0 ? s_val[cur][i - 1] : 0ull;
        const uint64_t cin = xh != 0 ? xv : carry + xv;
        const uint64_t next_carry = s_has[cur][C - 1] != 0 ? s_val[cur][C - 1] : carry + s_val[cur][C - 1];
        const uint32_t pl = i != 0 ? ((s_flags[i - 1] & kFieldsLastIn) != 0 ? 1u : 0u) : prev_last;
        const uint32_t next_last = (s_flags[C - 1] & kFieldsLastIn) != 0 ? 1u : 0u;
        // what the head line adds
        uint32_t hb = 0, he = 0;
        if (w < ca.parts) {
            const uint64_t first = ca.first, last = ca.last, T = cin + s.head_events;
            if (ca.merge) {
                if (cin <= first - 1 && T > first - 1) hb = 1;
            } else if (first >= 2) {
                if (cin <= first - 2 && T > first - 2) hb = 1;
            }
            if (last != 0) {
                if (!ca.merge) {
                    if (cin <= last - 1 && T > last - 1) he = 1;
                } else {
                    // the head's field ends close runs cin + 1 - cont .. cin + head_ends - cont; cont: its first byte goes on with a run
                    const uint64_t cont = (s.flags & kFieldsFirstIn) != 0 && pl != 0 ? 1u : 0u;
                    if (s.head_ends != 0 && last >= cin + 1 - cont && last <= cin + s.head_ends - cont) he = 1;
                }
            }
            if (s.nd != 0 || (s.flags & kFieldsVirtual) != 0) {                 // the head line ends here
                const bool sel = T >= (ca.merge ? first : first - 1);
                if (sel && (last == 0 || T < last)) he += 1;
                if (!sel && ca.keep) {
                    hb += 1;
                    he += 1;
                }
            }
        }
        const uint32_t nb = s.begins + hb, ne = s.ends + he;
        s_nb[0][i] = nb;
        s_ne[0][i] = ne;
        s_nd[0][i] = s.nd;
        __syncthreads();
        cur = 0;
        for (int d = 1; d < C; d <<= 1) {
            uint32_t vb = s_nb[cur][i], ve = s_ne[cur][i], vd = s_nd[cur][i];
            if (i >= d) {
                vb += s_nb[cur][i - d];
                ve += s_ne[cur][i - d];
                vd += s_nd[cur][i - d];
            }
            s_nb[cur ^ 1][i] = vb;
            s_ne[cur ^ 1][i] = ve;
            s_nd[cur ^ 1][i] = vd;
            __syncthreads();
            cur ^= 1;
        }
        if (w < ca.parts) {
            const FieldsPre p = {cin, lines + (s_nd[cur][i] - s.nd), rb + (s_nb[cur][i] - nb), re + (s_ne[cur][i] - ne), nb, ne, 0};
            ca.pre[w] = p;
        }
        carry = next_carry;
        prev_last = next_last;
        lines += s_nd[cur][C - 1];
        rb += s_nb[cur][C - 1];
        re += s_ne[cur][C - 1];
        __syncthreads();                                                        // (the next chunk writes the buffers read above)
    }
    if (i == 0) {
        ca.totals[0] = rb;
        ca.totals[1] = re;
        ca.totals[2] = lines + ((ca.sum[ca.parts - 1].flags & kFieldsVirtual) != 0 ? 1u : 0u);
    }
}

}  // namespace ss
