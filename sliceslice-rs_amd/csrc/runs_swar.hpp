// runs_swar.hpp - membership of four bytes at once in a range [lo, hi] of byte values, and the split of a set into its maximal ranges
// (include/sliceslice_hip_runs.h; used by runs_kernels.hpp on the device and by ss_runs.hip and tests/native/runs_host_check.cpp on
// the host).  Plain C++: no HIP header is included here, so a CPU program can sweep the test exhaustively.
//
// x >= c for every byte of a dword, exact for all 256 values and without a carry between bytes: with l = the low seven bits of a
// byte and c7 = those of c, l + (0x80 - c7) has bit 7 set iff l >= c7 (the sum is at most 0xFF).  Where c < 0x80 the byte is >= c
// iff its own bit 7 is set OR that test holds; where c >= 0x80 iff its bit 7 is set AND the test holds.  A range is
// (x >= lo) and not (x >= hi + 1); hi == 0xFF has no second test.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define SS_RUNS_HD __host__ __device__
#else
#define SS_RUNS_HD
#endif

namespace ss {

constexpr int kRunsMaxRanges = 4;               // SS_RUNS_MAX_RANGES

// The constants of one range, splatted over the four bytes of a dword.
struct RunsRange {
    uint32_t add_lo;        // 0x80 - (lo & 0x7F)
    uint32_t or_lo;         // 0x80 where lo < 0x80 (the byte's bit 7 alone settles it), else 0
    uint32_t add_hi;        // the same for hi + 1 ...
    uint32_t or_hi;
    uint32_t keep_hi;       // ... 0x80 where hi < 0xFF, 0 where there is no upper test
};

SS_RUNS_HD inline RunsRange runs_range(unsigned lo, unsigned hi)
{
    const unsigned c = (hi + 1u) & 0xFFu;
    RunsRange r;
    r.add_lo = (0x80u - (lo & 0x7Fu)) * 0x01010101u;
    r.or_lo = (lo & 0x80u) ? 0u : 0x80808080u;
    r.add_hi = (0x80u - (c & 0x7Fu)) * 0x01010101u;
    r.or_hi = (c & 0x80u) ? 0u : 0x80808080u;
    r.keep_hi = hi < 0xFFu ? 0x80808080u : 0u;
    return r;
}

// bit 7 of every byte of x that lies in the range (the other bits of the result are zero)
SS_RUNS_HD inline uint32_t runs_in_range4(uint32_t x, const RunsRange &r)
{
    const uint32_t l = x & 0x7F7F7F7Fu;
    const uint32_t a = l + r.add_lo, b = l + r.add_hi;
    const uint32_t ge_lo = (a & x) | ((a | x) & r.or_lo);
    const uint32_t ge_hi = ((b & x) | ((b | x) & r.or_hi)) & r.keep_hi;
    return ge_lo & ~ge_hi & 0x80808080u;
}

// The maximal ranges of a set (256 bits, byte b at bit b & 63 of word b >> 6), ascending: the first `capacity` go to lo / hi.
// Returns their number, 0 .. 128.
inline unsigned runs_ranges(const uint64_t *set, uint8_t *lo, uint8_t *hi, unsigned capacity)
{
    unsigned n = 0;
    for (unsigned b = 0; b < 256;) {
        if (((set[b >> 6] >> (b & 63)) & 1u) == 0) {
            ++b;
            continue;
        }
        unsigned e = b;
        while (e + 1 < 256 && ((set[(e + 1) >> 6] >> ((e + 1) & 63)) & 1u)) ++e;
        if (n < capacity) {
            lo[n] = (uint8_t)b;
            hi[n] = (uint8_t)e;
        }
        ++n;
        b = e + 1;
    }
    return n;
}

}  // namespace ss
