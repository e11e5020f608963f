// batched_types.hpp - what the many-problem kernels share: the records a batch is described by (BatchArgs, BatchDesc, BatchCold),
// the device functions that build and read them, and the launcher of the one kernel that two translation units launch.  No kernel
// is defined here: those of ss_search_batched / ss_find_batched / ss_batch_plan_* are in batched_kernels.hpp (ss_batched.hip), the
// all-matches ones in batched_all_kernels.hpp (scan_inst_all_batched.hip).
#pragma once
#include "scan_kernels.hpp"

namespace ss {

// A batch as the caller names it: every problem is a pair of ranges (begin[i], end[i]) into the two blobs - CSR callers pass
// (off, off + 1); ranges may alias (many needles, one haystack).
struct BatchArgs {
    const uint8_t *haystacks;
    const uint64_t *hay_begin, *hay_end;
    const uint8_t *needles;
    const uint64_t *needle_begin, *needle_end;
    const uint64_t *position;   // may be null: n_i - 1
    int *found;                 // search: one int32 flag per problem
    uint64_t *best;             // find (ss_find_batched): one uint64 leftmost offset per problem (all ones = absent); else null
};
constexpr int kBadPosition = -1;   // SS_BATCH_BAD_POSITION: flag of a problem whose position breaks the with_position rules

// ---- K4, planned form: a one-lane-per-problem plan kernel + the scan grid ------------------------------------
// A scan kernel that rebuilds its problem descriptor in every workgroup - ranges -> needle bytes -> first haystack load - has a
// chain of three dependent memory round trips (3-4 us under load) in front of every slice, which is why it only did well
// when a slice was long (4,096 x 1 MiB in ~10-tile slices: 0.88-0.90 of the HBM peak; 1,024 x 1 MiB in 8-tile slices: 0.73).
// Here the descriptors are built ONCE per problem by batch_plan_kernel (one lane per problem; it also writes the initial
// flag, so it replaces the memset launch), 64 bytes each, and a scan workgroup starts with ONE scalar load
// (s_load_dwordx16 of its problem's descriptor, issued together with the entry poll of the problem's flag) before its first
// haystack load - one round trip more than scan_kernel, whose descriptor travels in the kernel arguments.  With the start-up
// chain gone, slices can be short (kPlanMinTiles) and the grid generous: surplus slices leave after that one scalar load.
struct __attribute__((aligned(64))) BatchDesc {
    const uint8_t *base;       // 16-byte-aligned start of the filter stream: hay + anchor - mis
    uint64_t end;              // candidate offsets (0: nothing to scan - trivial problem, answered by the plan kernel)
    uint64_t nchunks_all;
    uint64_t n;                // needle length
    uint64_t needle_off;       // offset of the needle in the needle blob
    uint64_t anchor;           // index of the first filter byte in the needle
    uint64_t per;              // active slices of the problem << 32 | tiles per slice (both < 2^32: the grid is one-dimensional)
    uint32_t bytes;            // needle[anchor] | second byte << 8 | third byte << 16 | (one-byte needle) << 24
    uint32_t shifts;           // mis | r << 4 | Q << 6 | r3 << 8 | q3 << 10
};
static_assert(sizeof(BatchDesc) == 64, "one scalar load (s_load_dwordx16) per workgroup");
// The cold part of a problem - what verification needs - where it is written ahead of the scan (see ColdInPlan / ColdInCall below).
struct __attribute__((aligned(64))) BatchCold {
    uint64_t order_idx[2], order_val[2];       // as Problem::order_idx / order_val (build_refine_order)
    uint32_t tail16[4];                        // as Problem::tail16
    uint32_t norder, exact_len;
    // The problem's STATE while a scan runs lives here too - a line of its own per pair of problems, not one of 16 or 32 words of
    // an array: every wave polls its problem's word once per tile, the resident workgroups of a problem-major launch belong to a
    // few dozen consecutive problems, and with their words in ONE cache line every match (an atomic on that line) sent the polls of
    // all of them to memory - 1,024 x 1 MiB with every needle present ran 0.23-0.29 ms where the full scan takes 0.155.
    //   unplanned bool calls: pad[1] = the found flag the waves poll and raise (the caller's output is written behind it)
    //   unplanned find calls: pad[0..1] = one uint64, the leftmost offset so far (the caller's output is lowered behind it)
    //   plans:                not here - a plan's problems have a PlanState of their own (two words, one per run parity: below)
    uint32_t pad[2];
};
static_assert(sizeof(BatchCold) == 64, "one scalar load");

__host__ __device__ constexpr inline int rarity_class4(uint8_t b)
{
    const int r = byte_rarity_rank(b);
    return r < 64 ? 0 : (r < 128 ? 1 : (r < 192 ? 2 : 3));
}
// The four classes as two bit planes of 256 bits each (8 dwords per plane): no table in memory, no branches - the plan kernel
// fills its LDS table from these constants.
struct ClassPlanes {
    uint32_t lo[8], hi[8];
};
constexpr ClassPlanes make_class_planes()
{
    ClassPlanes p = {};
    for (int b = 0; b < 256; ++b) {
        const int c = rarity_class4((uint8_t)b);
        if (c & 1) p.lo[b >> 5] |= 1u << (b & 31);
        if (c & 2) p.hi[b >> 5] |= 1u << (b & 31);
    }
    return p;
}
constexpr uint32_t kClassNone = 255;            // above every class of either table

// What the plan kernel tells the host about a plan's problems (ss_batch_plan_create sizes the grid of the runs from it).
struct PlanStats {
    uint32_t max_slices;       // the most active slices any problem got
    uint32_t max_tiles;        // the longest scan, in tiles (saturating)
    uint64_t total_tiles;
};

// One problem's descriptor (and, for the unplanned calls, its initial output); returns its number of active slices.
__device__ __forceinline__ uint32_t plan_one(const BatchArgs &a, uint64_t prob, uint64_t h0, uint64_t h1, uint64_t n0, uint64_t n1, uint64_t given,
                                             BatchDesc *descs, uint32_t nslices, uint32_t min_tiles, int tile_pieces, const uint8_t *s_class,
                                             uint64_t *tiles_out, bool free_pair, BatchCold *colds)
{
    *tiles_out = 0;
    const uint64_t len = h1 - h0, n = n1 - n0;
    const uint64_t position = (a.position && n) ? given : n - 1;
    BatchDesc d;
    d.base = nullptr;
    d.end = d.nchunks_all = 0;
    d.n = n;
    d.needle_off = n0;
    d.anchor = 0;
    d.per = 0;                                      // no active slice
    d.bytes = d.shifts = 0;
    BatchCold lite;                                 // (unplanned calls) the needle's dwords where they are at hand: see ColdInCall
    lite.order_idx[0] = lite.order_idx[1] = lite.order_val[0] = lite.order_val[1] = 0;
    lite.tail16[0] = lite.tail16[1] = lite.tail16[2] = lite.tail16[3] = 0;
    lite.norder = lite.exact_len = 0;
    lite.pad[0] = lite.pad[1] = 0;
    int flag = 0;
    if (n == 0) {
        flag = 1;                                   // N0: found everywhere (x86.rs:500)
    } else if (n == 1 ? position != 0 : position >= n) {
        flag = kBadPosition;                        // the reference panics building this searcher (x86.rs:300, 473)
    } else if (len >= n) {
        const uint8_t *needle = a.needles + n0;
        uint64_t anchor = 0;
        if (position >= 16) {
            uint32_t cls[15];
#pragma unroll
            for (int k = 0; k < 15; ++k) cls[k] = needle[position - 15 + k];
#pragma unroll
            for (int k = 0; k < 15; ++k) cls[k] = s_class[cls[k]];
            uint32_t best_cls = kClassNone;
#pragma unroll
            for (int k = 0; k < 15; ++k) {          // later bytes win ties: the partner closest to `position`
                const bool better = cls[k] <= best_cls;
                best_cls = better ? cls[k] : best_cls;
                anchor = better ? position - 15 + k : anchor;
            }
        }
        uint32_t s2 = (uint32_t)(position - anchor);            // distance between the two filter bytes: 0 .. 15
        const uint32_t lim = n - anchor < 16 ? (uint32_t)(n - anchor) : 16u;
        uint32_t fb[16], cls[16];
#pragma unroll
        for (uint32_t k = 0; k < 16; ++k) fb[k] = needle[anchor + (k < lim ? k : 0u)];
#pragma unroll
        for (uint32_t k = 0; k < 16; ++k) cls[k] = s_class[fb[k]];
        if (free_pair && anchor == 0 && position == n - 1) {
            // nobody chose `position` (it is the default, the last byte) and the classes are the haystacks' own: the partner of
            // needle[0] is the rarest of the 15 bytes behind it, as ss_searcher_new would have it, the later one among equals
            uint32_t bc = kClassNone;
#pragma unroll
            for (uint32_t k = 1; k < 16; ++k) {
                const bool better = k < lim && cls[k] <= bc;
                bc = better ? cls[k] : bc;
                s2 = better ? k : s2;
            }
        }
        uint32_t p3 = s2, best_cls = kClassNone;
#pragma unroll
        for (uint32_t k = 1; k < 16; ++k) {         // the rarest of the 15 bytes behind the anchor, later ones winning ties
            const bool better = k < lim && k != s2 && cls[k] <= best_cls && n - anchor >= 3;
            best_cls = better ? cls[k] : best_cls;
            p3 = better ? k : p3;
        }
        if (p3 / 4 > s2 / 4) {                      // the kernels want the third byte's dword not behind the second's
            const uint32_t t = p3;
            p3 = s2;
            s2 = t;
        }
        uint32_t b2 = 0, b3 = 0;
#pragma unroll
        for (uint32_t k = 0; k < 16; ++k) {         // fb[s2], fb[p3] without a dynamic index (scratch)
            b2 = k == s2 ? fb[k] : b2;
            b3 = k == p3 ? fb[k] : b3;
        }
        if (anchor == 0 && n >= 2 && n <= 16) {
            // the whole needle sits in fb[0 .. n): the dwords of the in-register compare, no byte in front of the first filter byte.
            // (Measured against the lazy form in one process, profiles/r05/ab_call_cold.jsonl: the reference's i386 loop 0.135 ms a
            // call instead of 0.145; every second needle present, 16,384 x 64 KiB 0.168 instead of 0.207, 65,536 x 16 KiB 0.336
            // instead of 0.492; without matches the same.  Round-robin launches - few problems, two dozen workgroups each - gain
            // nothing from it, and lost 4-8 % as long as their state words shared cache lines: see BatchCold.)
#pragma unroll
            for (int j = 0; j < 4; ++j)
                lite.tail16[j] = (4u * j + 0 < n ? fb[4 * j] : 0u) | ((4u * j + 1 < n ? fb[4 * j + 1] : 0u) << 8) |
                                 ((4u * j + 2 < n ? fb[4 * j + 2] : 0u) << 16) | ((4u * j + 3 < n ? fb[4 * j + 3] : 0u) << 24);
            lite.exact_len = (uint32_t)n;
        }
        const uint8_t *hf = a.haystacks + h0 + anchor;
        const uint32_t mis = (uint32_t)((uintptr_t)hf & 15);
        d.base = hf - mis;
        d.end = len - n + 1;
        d.nchunks_all = (mis + len - anchor + 15) / 16;
        d.anchor = anchor;
        d.bytes = fb[0] | (b2 << 8) | (b3 << 16) | (n == 1 ? 1u << 24 : 0u);
        d.shifts = mis | ((s2 % 4) << 4) | ((s2 / 4) << 6) | ((p3 % 4) << 8) | ((p3 / 4) << 10);
        const uint64_t npieces = ((mis + d.end + 15) / 16 + 63) / 64;
        const uint64_t ntiles = (npieces + tile_pieces - 1) / tile_pieces;
        uint64_t eff = (ntiles + min_tiles - 1) / min_tiles;
        eff = eff < nslices ? (eff ? eff : 1) : nslices;
        d.per = (eff << 32) | ((ntiles + eff - 1) / eff);
        *tiles_out = ntiles;
    }
    if (colds) {                                           // (unplanned calls: ColdInCall; the state word idle)
        lite.pad[0] = lite.pad[1] = a.best ? ~0u : 0u;
        colds[prob] = lite;
    }
    if (d.per == 0) d.shifts = (uint32_t)flag;             // no scan: the answer travels in the descriptor too (plan runs)
    if (a.best) a.best[prob] = n == 0 ? 0ull : ~0ull;      // the empty needle matches at offset 0 of every haystack
    else if (a.found) a.found[prob] = flag;
    descs[prob] = d;
    return (uint32_t)(d.per >> 32);
}

// What a scan workgroup does with its problem's descriptor (scan_batched_plan_kernel, scan_all_batched_kernel).  The hot fields
// are pinned in scalar registers in front of the kernel's first store: a load the compiler sinks behind a store cannot go through
// the scalar cache any more, so it became a per-lane load and everything computed from it - tile bounds, loop control, addresses -
// per-lane arithmetic under exec masks (101 VGPRs, and 311 us where the unpinned kernel takes 154 on 1,024 x 1 MiB).
__device__ __forceinline__ void pin_hot_fields(BatchDesc &d)
{
    uint64_t base = reinterpret_cast<uint64_t>(d.base);
    __asm__ volatile("" : "+s"(base), "+s"(d.end), "+s"(d.nchunks_all), "+s"(d.per), "+s"(d.bytes), "+s"(d.shifts));
    d.base = reinterpret_cast<const uint8_t *>(base);
}
// The hot fields of the Problem; the cold ones are re-read from the descriptor by the waves that need them (ColdFields below).
__device__ __forceinline__ void hot_problem(const BatchDesc &d, uint32_t mis, uint64_t npieces, Problem &pr)
{
    pr.base = d.base;
    pr.nchunks_all = d.nchunks_all;
    pr.npieces = npieces;
    pr.d = 0;
    pr.find_base = 0;
    pr.mis = mis;
    pr.r = (d.shifts >> 4) & 3;
    pr.n0x4 = 0x01010101u * (d.bytes & 0xFF);
    pr.nlx4 = 0x01010101u * ((d.bytes >> 8) & 0xFF);
    pr.n3x4 = 0x01010101u * ((d.bytes >> 16) & 0xFF);
    pr.r3 = (d.shifts >> 8) & 3;
    pr.q3 = (d.shifts >> 10) & 3;
    pr.epoch = 1;
    pr.flags = 0;
    pr.q = (d.shifts >> 6) & 3;
}

// The cold fields of a planned problem, re-read from its descriptor by the waves that need them (scan_tiles' ColdT).
struct ColdFields {
    const uint8_t *hay, *needle;
    uint64_t n, end;
    uint32_t norder, exact_len;
    uint64_t order_idx[2], order_val[2];
    uint32_t tail16[4];
    int *host_flag;
    uint32_t *tally;                              // (ColdInPlan, plans that hold two layouts) the run's count of found problems; else null
    uint64_t far_off;
    uint32_t ready;                               // (ColdInCall) the record holds the needle's dwords: nothing to build
    __device__ __forceinline__ const ColdFields *operator->() const { return this; }
};
// A PLAN carries the cold part ready-made: what a wave of the unplanned kernel builds when it first meets a candidate - the
// second-level schedule (up to 15 further needle bytes, rarest first) and, for needles that end within 16 bytes of the first filter
// byte, the needle's dwords for the in-register compare - costs it a dependent round trip to the needle bytes plus a few hundred
// operations, once per wave and WORKGROUP: nothing on random bytes, where next to no wave meets a candidate; where the needles ARE
// there (the reference's bench: every word occurs in the text) it sits on the path of every problem's answer - 65,536 problems of
// 16 KiB, every second needle present: 0.447 ms a run, 0.271 with the cold part ready-made - and on text full of near misses it is
// paid by every other workgroup.  batch_cold_kernel (one LANE per problem, once per plan) writes one 64-byte BatchCold per
// problem; a wave then needs one more load.
// The unplanned calls' form: the plan kernel of a call writes a record too, but only what costs it nothing - for a needle of up to
// 16 bytes whose first filter byte is needle[0] (every needle of that length unless the caller chose a position of 16 or more) the
// needle's dwords are already in its registers: tail16, exact_len (non-zero says: usable as it is), an empty schedule.  A wave that meets a candidate looks
// there first and builds the cold part itself (scan_tiles, BUILD_ORDER) only when the record says it must.
// The cold fields as a ready-made record holds them (a plan's, or the all-matches calls'): no output to write behind a state word, no
// tally.  The functors below override what differs.
__device__ __forceinline__ ColdFields read_cold(const BatchDesc *q, const BatchCold *c, const uint8_t *needles)
{
    __asm__ volatile("" : "+s"(q), "+s"(c));        // opaque: the loads stay in the cold path
    ColdFields f;
    f.hay = q->base + (q->shifts & 15) - q->anchor;
    f.needle = needles + q->needle_off;
    f.n = q->n;
    f.end = q->end;
    f.norder = c->norder;
    f.exact_len = c->exact_len;
    f.order_idx[0] = c->order_idx[0]; f.order_idx[1] = c->order_idx[1];
    f.order_val[0] = c->order_val[0]; f.order_val[1] = c->order_val[1];
    f.tail16[0] = c->tail16[0]; f.tail16[1] = c->tail16[1]; f.tail16[2] = c->tail16[2]; f.tail16[3] = c->tail16[3];
    f.host_flag = nullptr;
    f.tally = nullptr;
    f.far_off = 0;
    f.ready = 1;
    return f;
}
struct ColdInCall {
    static constexpr bool kHasOrder = false;
    static constexpr bool kMaybeOrder = true;
    const BatchDesc *dp;
    const BatchCold *cp;
    const uint8_t *needles;
    void *out_word;                                 // the caller's output of this problem - int flag or uint64 offset: the wave that finds writes it
    __device__ __forceinline__ ColdFields operator()() const
    {
        ColdFields f = read_cold(dp, cp, needles);
        f.norder = 0;                               // an empty schedule
        f.order_idx[0] = f.order_idx[1] = f.order_val[0] = f.order_val[1] = 0;
        f.host_flag = static_cast<int *>(out_word);
        f.ready = f.exact_len;                      // (the plan kernel sets it only where it left the dwords)
        return f;
    }
};
// MULTI = false is also the all-matches scan's form (scan_all_batched_kernel: no state word, out_word and tally null).
template <bool MULTI>
struct ColdInPlanT {
    static constexpr bool kHasOrder = true;
    static constexpr bool kMaybeOrder = false;
    static constexpr bool kSingleLaunchPlan = MULTI;  // scan_tiles: state word first, the caller's output behind it, the tally
    const BatchDesc *dp;
    const BatchCold *cp;
    const uint8_t *needles;
    void *out_word;                                 // problems scanned by several workgroups: the caller's output of this problem; else null
    uint32_t *tally;
    __device__ __forceinline__ ColdFields operator()() const
    {
        ColdFields f = read_cold(dp, cp, needles);
        f.host_flag = MULTI ? static_cast<int *>(out_word) : nullptr;
        f.tally = MULTI ? tally : nullptr;
        return f;
    }
};

// batch_cold_kernel (batched_kernels.hpp: one lane per problem, the cold records of `count` descriptors) lives in ss_batched.hip;
// this is how ss_batch_plan_create and the batched all-matches calls (scan_inst_all_batched.hip, same library) launch it.
// `cls`: the haystacks' own 256 rarity classes, or null for the static four; `find`: the idle state word is all ones.
hipError_t launch_batch_cold(const BatchArgs &a, const BatchDesc *descs, uint64_t count, BatchCold *colds, const uint8_t *cls, int find,
                             hipStream_t st);

}  // namespace ss
