// anyof_segments.hpp - the index arithmetic of the union of ascending lists of line numbers (include/sliceslice_hip_anyof.h): plain
// 64-bit arithmetic for the host and the device, so that a host program can run it (tests/native/anyof_segments_check.cpp).
//
// The numbers 1 .. limit are cut into SEGMENTS of L consecutive numbers (L = SS_ANYOF_SEGMENT_LINES in the library; the host check
// also runs a small L).  Segment g holds g * L + 1 .. min((g + 1) * L, limit); number v sits at bit (v - 1) % 32 of word
// ((v - 1) % L) / 32 of its segment's bitmap.  A list contributes to a segment the SLICE of its entries that lie in it, found by
// two binary searches; every entry of a slice is still tested against the segment before its bit is set, so that lists that break
// the contract (not ascending) can set no bit outside the bitmap.  The bits of a word leave in ascending order for consecutive
// output slots, and no slot at or above the capacity is written.
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SS_ANY_HD __host__ __device__ inline
#else
#define SS_ANY_HD inline
#endif

namespace ss {

template <uint64_t L>
struct AnySegments {
    static_assert(L >= 1, "a segment holds a number");
    static constexpr uint64_t kWords = (L + 31) / 32;           // 32-bit words of a segment's bitmap

    // segments that 1 .. limit need
    static SS_ANY_HD uint64_t segments(uint64_t limit) { return limit / L + (limit % L ? 1u : 0u); }
    // the first and the last number of segment g (g < segments(limit)); neither can overflow: both are <= limit
    static SS_ANY_HD uint64_t first(uint64_t g) { return g * L + 1; }
    static SS_ANY_HD uint64_t valid(uint64_t g, uint64_t limit) { return limit - g * L < L ? limit - g * L : L; }    // numbers in it: the cut of the last one
    static SS_ANY_HD uint64_t last(uint64_t g, uint64_t limit) { return g * L + valid(g, limit); }
    // where number v (>= 1) sits
    static SS_ANY_HD uint64_t segment_of(uint64_t v) { return (v - 1) / L; }
    static SS_ANY_HD uint32_t word_of(uint64_t v) { return (uint32_t)(((v - 1) % L) / 32); }
    static SS_ANY_HD uint32_t bit_of(uint64_t v) { return 1u << (uint32_t)(((v - 1) % L) % 32); }
    // the number at bit b of word w of segment g
    static SS_ANY_HD uint64_t number_at(uint64_t g, uint32_t w, uint32_t b) { return g * L + 1 + (uint64_t)w * 32 + b; }
    // the bits of word w that stand for numbers of a segment with `valid` numbers
    static SS_ANY_HD uint32_t word_mask(uint32_t w, uint64_t valid)
    {
        const uint64_t lo = (uint64_t)w * 32;
        if (valid >= lo + 32) return ~0u;
        if (valid <= lo) return 0u;
        return (1u << (uint32_t)(valid - lo)) - 1u;
    }
    // the bits of word w that leave: the set ones, or with `complement` the clear ones among the valid
    static SS_ANY_HD uint32_t out_bits(uint32_t word, uint32_t w, uint64_t valid, int complement)
    {
        return (complement ? ~word : word) & word_mask(w, valid);
    }
};

// the first index in [lo, hi) whose entry is >= v (hi: none); terminates inside [lo, hi] whatever the order of the entries is
SS_ANY_HD uint64_t any_lower(const uint64_t *list, uint64_t lo, uint64_t hi, uint64_t v)
{
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (list[mid] < v) lo = mid + 1; else hi = mid;
    }
    return lo;
}
// the first index in [lo, hi) whose entry is > v
SS_ANY_HD uint64_t any_upper(const uint64_t *list, uint64_t lo, uint64_t hi, uint64_t v)
{
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (list[mid] <= v) lo = mid + 1; else hi = mid;
    }
    return lo;
}

struct AnySlice {
    uint64_t lo, hi;            // entries [lo, hi) of the numbers; lo <= hi always
};
// The entries of list [b, e) that lie in first .. last (first <= last).
SS_ANY_HD AnySlice any_slice(const uint64_t *numbers, uint64_t b, uint64_t e, uint64_t first, uint64_t last)
{
    AnySlice s;
    s.lo = any_lower(numbers, b, e, first);
    s.hi = any_upper(numbers, s.lo, e, last);
    return s;
}
// an entry of a slice sets a bit only when it really lies in the segment (it does, when the list ascends)
SS_ANY_HD bool any_inside(uint64_t v, uint64_t first, uint64_t last) { return v >= first && v <= last; }

SS_ANY_HD uint32_t any_popc(uint32_t x)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return (uint32_t)__popc(x);
#else
    return (uint32_t)__builtin_popcount(x);
#endif
}

// Writes the numbers of `bits` (bit b: base + b) ascending to out[slot], out[slot + 1], ... and returns the slot behind them; no
// slot at or above the capacity is written.
SS_ANY_HD uint64_t any_emit_word(uint32_t bits, uint64_t base, uint64_t slot, uint64_t capacity, uint64_t *out)
{
    for (; bits; bits &= bits - 1, ++slot)
        if (slot < capacity) out[slot] = base + (uint32_t)__builtin_ctz(bits);
    return slot;
}

}  // namespace ss
