// lines_tiles.hpp - the per-tile half of the matching-lines scan (include/sliceslice_hip_lines.h): what scan_tiles<..., LINES = true>
// (scan_kernels.hpp) does with a tile's delimiter bytes and match masks.  The kernels around it are in lines_kernels.hpp.
//
// Everything here works in STREAM coordinates - byte a of the filter stream is the byte the wave holds in its registers, i.e.
// hay[a + hshift] (hshift = index of the first filter byte - misalignment).  A match's flag sits at its first filter byte, a
// delimiter at itself, and a needle that could match holds no delimiter, so "match before delimiter" is the order of the two
// register positions.
//
// Forward only: a line belongs to the delimiter that closes it and is counted (emitted) iff a match has been seen since the
// delimiter before.  A part (lane, piece, wave-tile, workgroup) is summed up as
//     has_delim | head_match (a match before its first delimiter - anywhere if it has none) | tail_match (one after its last),
//     the number of delimiters, the number of matching lines closed inside NOT counting the first delimiter's line (whether that
//     one matches depends on what came before), and the last delimiter,
// and parts combine associatively: the first delimiter's line of b matches iff a.tail_match || b.head_match.
// Within a lane (16 bytes) and within a piece (64 lanes) the combine is ONE addition: with Z = the non-delimiter positions and M
// the match positions (+ the carry-in at the bottom), the carries of Z + M run through the non-delimiters behind every match and
// stop at the next delimiter, so (Z + M) & ~Z marks exactly the delimiters that close a matching line.
#pragma once
#include "scan_filters.hpp"

namespace ss {

constexpr int kLineTilesPerBlock = 4;       // tiles per workgroup whose wave summaries a workgroup keeps in LDS (the host launches <= this)
constexpr uint32_t kLineHas = 1u, kLineHead = 2u, kLineTail = 4u;

// A contiguous part of the view, as the scan leaves it in memory: one per workgroup (and one each for the bytes in front of and
// behind the filter stream).  No delimiter: head == tail == "a match anywhere".
struct LineSum {
    uint64_t ndelim;
    uint64_t closed;        // matching lines closed inside, not counting the first delimiter's line
    uint64_t last;          // hay index of the last delimiter + 1 (the first byte of the line behind it); 0: none
    uint32_t flags;         // kLineHas | kLineHead | kLineTail
    uint32_t pad;
};
// What has happened in front of a part.
struct LinePre {
    uint64_t ndelim;        // delimiters so far
    uint64_t rank;          // matching lines closed so far
    uint64_t last;          // first byte of the line that is open (0: the view's first line)
    uint32_t carry;         // a match since the last delimiter
    uint32_t closes;        // matching lines the part itself closes
};

__device__ __forceinline__ LineSum line_combine(const LineSum &a, const LineSum &b)
{
    // (branch-free on purpose: the fields of a part without a delimiter are zero, and selecting whole structs ends up in scratch memory)
    const bool ha = (a.flags & kLineHas) != 0, hb = (b.flags & kLineHas) != 0;
    const bool a_head = (a.flags & kLineHead) != 0, a_tail = (a.flags & kLineTail) != 0;
    const bool b_head = (b.flags & kLineHead) != 0, b_tail = (b.flags & kLineTail) != 0;
    LineSum r;
    r.ndelim = a.ndelim + b.ndelim;
    r.closed = a.closed + b.closed + ((ha && hb && (a_tail || b_head)) ? 1u : 0u);
    r.last = hb ? b.last : a.last;
    const bool head = ha ? a_head : (a_head || b_head);
    const bool tail = hb ? b_tail : (ha ? (a_tail || b_head) : (a_head || b_head));
    r.flags = ((ha || hb) ? kLineHas : 0u) | (head ? kLineHead : 0u) | (tail ? kLineTail : 0u);
    r.pad = 0;
    return r;
}

// state behind `e`, given the state in front of it; returns the number of matching lines e closes
__device__ __forceinline__ uint64_t line_advance(LinePre &s, const LineSum &e)
{
    if ((e.flags & kLineHas) == 0) {
        s.carry |= (e.flags & kLineHead) ? 1u : 0u;
        return 0;
    }
    const uint64_t c = e.closed + ((s.carry | (e.flags & kLineHead)) ? 1u : 0u);
    s.rank += c;
    s.ndelim += e.ndelim;
    s.last = e.last;
    s.carry = (e.flags & kLineTail) ? 1u : 0u;
    return c;
}

// (zero_bytes_exact - bit 7 of every byte that is zero, exactly - is scan_filters.hpp's: the case fold uses it too)

// The delimiters of a chunk in the TRANSPOSED layout the flag words have (verify_flags_walk): byte t of dword j at bit 8t + j.
__device__ __forceinline__ uint32_t delimiter_bits(const u32x4 &A, uint32_t dx4)
{
    return (zero_bytes_exact(A.x ^ dx4) >> 7) | (zero_bytes_exact(A.y ^ dx4) >> 6) | (zero_bytes_exact(A.z ^ dx4) >> 5) |
           (zero_bytes_exact(A.w ^ dx4) >> 4);
}

// transposed -> address order (byte k of the chunk at bit k) and back
__device__ __forceinline__ uint32_t line_ordered(uint32_t m)
{
    uint32_t r = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) r |= (((((m >> j) & 0x01010101u) * 0x01020408u) >> 24) & 0xFu) << (4 * j);
    return r;
}
__device__ __forceinline__ uint32_t line_transposed(uint32_t v)
{
    uint32_t r = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int t = 0; t < 4; ++t) r |= ((v >> (4 * j + t)) & 1u) << (8 * t + j);
    return r;
}

// What a lines launch hands to scan_tiles as its sink (a local of lines_scan_kernel).
struct LineTiles {
    uint32_t delim_x4;
    uint64_t dlo, dhi;          // stream positions of the view's first byte and of its end: delimiters outside do not count
    int64_t hshift;             // hay index = stream position + hshift
    bool emit;                  // wave-uniform: write records instead of summing up
    uint64_t tile0;             // the workgroup's first tile
    // summing up: per lane, over all of the wave's tiles
    uint32_t lane_ndelim, lane_closed;
    // LDS: one entry per (tile of the workgroup, wave) when summing up, per wave when emitting
    uint64_t *s_last;
    uint32_t *s_flags, *s_nd, *s_cl;
    // emitting: the state in front of the workgroup's next tile (workgroup-uniform), and the caller's arrays
    LinePre at;
    uint64_t *begin, *end, *number;
    uint64_t capacity;
};

// bytes outside the view are masked out of the delimiter masks of a wave's U pieces
template <int U>
__device__ __forceinline__ void line_clip(uint64_t chunk0, int lane, const LineTiles &lt, uint32_t (&dm)[U])
{
    if (chunk0 * 16 < lt.dlo || (chunk0 + 64 * U) * 16 > lt.dhi) {           // wave-uniform: the view's first and last tiles
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const uint64_t a = (chunk0 + 64 * u + lane) * 16;
            const uint32_t lo = lt.dlo > a ? (lt.dlo - a >= 16 ? 16u : (uint32_t)(lt.dlo - a)) : 0u;
            const uint32_t hi = lt.dhi > a ? (lt.dhi - a >= 16 ? 16u : (uint32_t)(lt.dhi - a)) : 0u;
            const uint32_t v = hi > lo ? ((1u << hi) - 1u) & ~((1u << lo) - 1u) : 0u;
            dm[u] &= line_transposed(v);
        }
    }
}

// the delimiter masks of a wave's U pieces (transposed layout), bytes outside the view masked out
template <int U>
__device__ __forceinline__ void line_capture(const u32x4 (&A)[U], uint64_t chunk0, int lane, const LineTiles &lt, uint32_t (&dm)[U])
{
#pragma unroll
    for (int u = 0; u < U; ++u) dm[u] = delimiter_bits(A[u], lt.delim_x4);
    line_clip<U>(chunk0, lane, lt, dm);
}

// a lane's match mask in address order: the offsets verified on behalf of the next lane's chunk (exact_verify_piece_all, bits
// 16 ..) go back to the lane that holds them
__device__ __forceinline__ uint32_t line_matches(uint32_t mk, int lane)
{
    const uint32_t up = (uint32_t)__shfl_up((int)(mk >> 16), 1u, kWave);
    return (mk & 0xFFFFu) | (lane == 0 ? 0u : up);
}

// One piece: dm / mm = a lane's delimiters / matches in address order, c = "a match since the last delimiter" in front of the piece
// (wave-uniform; updated to the same behind it).  Returns the lane's delimiters that close a matching line; HD = lanes with a delimiter.
__device__ __forceinline__ uint32_t line_piece(uint32_t dm, uint32_t mm, uint32_t &c, int lane, uint64_t &HD)
{
    HD = __ballot(dm != 0);
    const uint32_t behind = dm ? mm >> (32 - __builtin_clz(dm)) : mm;           // matches behind the lane's last delimiter
    const uint64_t TM = __ballot(behind != 0);
    // lanes a pending match enters: it starts behind every lane of TM (and in front of lane 0 with c) and runs through the lanes
    // without a delimiter into the first one that has one
    const uint64_t S = (TM << 1) | c, Z = ~HD;
    const uint64_t C = (((S & Z) + Z) ^ Z) | S;
    const uint32_t cin = (uint32_t)(C >> lane) & 1u;
    const uint32_t Zl = ((~dm & 0xFFFFu) << 1) | 1u, Ml = ((mm & ~dm & 0xFFFFu) << 1) | cin;
    c = (uint32_t)((TM | (C & Z)) >> 63);
    return ((Zl + Ml) >> 1) & dm;
}

// hay index + 1 of the wave's last delimiter in a piece whose lanes HD (not 0) hold one
__device__ __forceinline__ uint64_t line_last(uint64_t HD, uint32_t dm_ordered, uint64_t piece_chunk, const LineTiles &lt)
{
    const int l = 63 - __builtin_clzll(HD);
    const uint32_t d = (uint32_t)__builtin_amdgcn_readlane((int)dm_ordered, l);
    return (uint64_t)((int64_t)((piece_chunk + (uint64_t)l) * 16 + (uint64_t)(31 - __builtin_clz(d))) + lt.hshift) + 1;
}

// The summary of a wave's part of a tile, pending match in front of it taken as none: flags and last delimiter are returned, the
// lane's delimiters and closed lines (the first delimiter's line included when the part's head matches) are added to nd / cl.
template <int U>
__device__ __forceinline__ uint32_t line_wave_summary(const LineTiles &lt, const uint32_t (&dmT)[U], const uint32_t (&mk)[U],
                                                      uint64_t chunk0, int lane, uint64_t &last, uint32_t &nd, uint32_t &cl)
{
    uint32_t anym = 0;
#pragma unroll
    for (int u = 0; u < U; ++u) {
        anym |= mk[u];
        nd += (uint32_t)__builtin_popcount(dmT[u]);
    }
    last = 0;
    if (__ballot(anym != 0) == 0) {
        // no match (the common tile): delimiters are counted in any order, and only the last one is located
#pragma unroll
        for (int u = U - 1; u >= 0; --u) {
            const uint64_t HD = __ballot(dmT[u] != 0);
            if (HD != 0 && last == 0) {
                const int l = 63 - __builtin_clzll(HD);
                const uint32_t d = line_ordered((uint32_t)__builtin_amdgcn_readlane((int)dmT[u], l));
                last = (uint64_t)((int64_t)((chunk0 + 64 * u + (uint64_t)l) * 16 + (uint64_t)(31 - __builtin_clz(d))) + lt.hshift) + 1;
            }
        }
        return last ? kLineHas : 0u;
    }
    uint32_t c = 0, head = 0, seen = 0;
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const uint32_t dm = line_ordered(dmT[u]), mm = line_matches(mk[u], lane);
        if (!seen) {
            // a match in front of the part's first delimiter: the lanes up to the first one that has a delimiter, that lane's
            // matches below its first delimiter
            const uint64_t HM = __ballot((mm & ((dm & (0u - dm)) - 1u)) != 0);
            const uint64_t HD0 = __ballot(dm != 0);
            const uint64_t upto = ((HD0 & (0ull - HD0)) << 1) - 1ull;
            if ((HM & upto) != 0) head = 1;
            seen = HD0 != 0;
        }
        uint64_t HD;
        cl += (uint32_t)__builtin_popcount(line_piece(dm, mm, c, lane, HD));
        if (HD != 0) last = line_last(HD, dm, chunk0 + 64 * u, lt);
    }
    return (seen ? kLineHas : 0u) | (head ? kLineHead : 0u) | (c ? kLineTail : 0u);
}

// The records of a wave's part of a tile, `s` = the state in front of it (wave-uniform).
// INVERT (the inverted emit kernels only, inverted_kernels.hpp): the delimiters that close a line WITHOUT a match are the selected
// ones - the complement of line_piece's within the delimiters - and a record's rank is the number of such lines in front of it,
// delimiters - matching lines, for the state, the lane prefix sums and the wave totals alike.  `s` arrives as the model's state.
template <int U, bool INVERT = false>
__device__ __forceinline__ void line_wave_emit(const LineTiles &lt, const uint32_t (&dmT)[U], const uint32_t (&mk)[U], uint64_t chunk0,
                                               int lane, LinePre s)
{
    uint32_t c = s.carry;
    if constexpr (INVERT) s.rank = s.ndelim - s.rank;
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const uint32_t dm = line_ordered(dmT[u]), mm = line_matches(mk[u], lane);
        uint64_t HD;
        const uint32_t cm = INVERT ? dm & ~line_piece(dm, mm, c, lane, HD) : line_piece(dm, mm, c, lane, HD);
        if (HD == 0) continue;                                                   // (nothing closes without a delimiter)
        const uint32_t ndl = (uint32_t)__builtin_popcount(dm), ncl = (uint32_t)__builtin_popcount(cm);
        const uint32_t ex_nd = wave_exclusive_sum(ndl, lane), ex_cl = wave_exclusive_sum(ncl, lane);
        const uint32_t tot_nd = (uint32_t)__builtin_amdgcn_readlane((int)(ex_nd + ndl), kWave - 1);
        const uint32_t tot_cl = (uint32_t)__builtin_amdgcn_readlane((int)(ex_cl + ncl), kWave - 1);
        const uint64_t a_lane = (chunk0 + 64 * u + (uint64_t)lane) * 16;
        if (tot_cl != 0 && s.rank < lt.capacity) {
            // the line open at the lane's first byte begins behind the last delimiter of the lanes below, or where the state says
            const uint64_t below = HD & ((1ull << lane) - 1ull);
            const int src = below ? 63 - __builtin_clzll(below) : 0;
            const uint32_t hb = dm ? 31u - (uint32_t)__builtin_clz(dm) : 0u;
            const uint32_t hb_src = (uint32_t)__shfl((int)hb, src, kWave);
            const uint64_t open = below ? (uint64_t)((int64_t)((chunk0 + 64 * u + (uint64_t)src) * 16 + hb_src) + lt.hshift) + 1 : s.last;
            uint32_t m = cm;
            uint64_t r = s.rank + ex_cl;
            while (m != 0 && r < lt.capacity) {
                const int b = __ffs((int)m) - 1;                                 // lowest first: address order within the lane
                m &= m - 1;
                const uint32_t lowd = dm & ((1u << b) - 1u);
                const uint64_t bg = lowd ? (uint64_t)((int64_t)(a_lane + (uint64_t)(31 - __builtin_clz(lowd))) + lt.hshift) + 1 : open;
                if (lt.begin) lt.begin[r] = bg;
                if (lt.end) lt.end[r] = (uint64_t)((int64_t)(a_lane + (uint64_t)b) + lt.hshift);
                if (lt.number) lt.number[r] = s.ndelim + ex_nd + (uint32_t)__builtin_popcount(lowd) + 1;
                ++r;
            }
        }
        s.last = line_last(HD, dm, chunk0 + 64 * u, lt);
        s.ndelim += tot_nd;
        s.rank += tot_cl;
    }
}

// End of a tile in a lines launch (scan_tiles' tile_done).  INVERT: an emit-only launch (lt.emit is not looked at, so that the
// summing half compiles away) whose waves write the lines they close that hold no match.
template <int U, bool INVERT = false>
__device__ __forceinline__ void line_tile_done(LineTiles &lt, const uint32_t (&dmT)[U], const uint32_t (&mk)[U], uint64_t tile,
                                               uint64_t chunk0, int lane, int wave, int wpb)
{
    uint64_t last;
    if (!INVERT && !lt.emit) {
        const uint32_t flags = line_wave_summary<U>(lt, dmT, mk, chunk0, lane, last, lt.lane_ndelim, lt.lane_closed);
        if (lane == 0) {
            const uint32_t slot = (uint32_t)(tile - lt.tile0) * kMaxWavesPerBlock + (uint32_t)wave;
            lt.s_last[slot] = last;
            lt.s_flags[slot] = flags;
        }
        return;
    }
    uint32_t nd = 0, cl = 0;
    const uint32_t flags = line_wave_summary<U>(lt, dmT, mk, chunk0, lane, last, nd, cl);
    const uint32_t wnd = wave_sum(nd), wcl = wave_sum(cl);
    if (lane == 0) {
        lt.s_last[wave] = last;
        lt.s_flags[wave] = flags;
        lt.s_nd[wave] = wnd;
        lt.s_cl[wave] = wcl;
    }
    __syncthreads();
    LinePre mine = lt.at;
    for (int w = 0; w < wpb; ++w) {
        if (w == wave) mine = lt.at;
        LineSum e;
        e.flags = lt.s_flags[w];
        e.ndelim = lt.s_nd[w];
        e.closed = (uint64_t)lt.s_cl[w] - ((e.flags & (kLineHas | kLineHead)) == (kLineHas | kLineHead) ? 1u : 0u);
        e.last = lt.s_last[w];
        (void)line_advance(lt.at, e);
    }
    __syncthreads();                                            // (the next tile rewrites the entries)
    if constexpr (INVERT) {
        // wcl holds the first delimiter's line when the wave's own head matches; a match pending in front of the wave makes it one too
        const uint32_t pending = (mine.carry && (flags & (kLineHas | kLineHead)) == kLineHas) ? 1u : 0u;
        if (wnd > wcl + pending) line_wave_emit<U, true>(lt, dmT, mk, chunk0, lane, mine);
    } else {
        if (wcl != 0 || (mine.carry && (flags & kLineHas))) line_wave_emit<U>(lt, dmT, mk, chunk0, lane, mine);
    }
}

}  // namespace ss
