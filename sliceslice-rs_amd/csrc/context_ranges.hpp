// context_ranges.hpp - which output lines an entry of a context call owns (include/sliceslice_hip_context.h): plain 64-bit
// arithmetic for the host and the device, so that a host program can run it (tests/native/context_ranges_check.cpp).
//
// The selected line numbers s_0 < s_1 < ... (1-based) with `before` = b and `after` = a print the union of
// [max(1, s - b), min(N, s + a)].  Entry i OWNS the lines from
//     max(1, s_i - b, min(s_{i-1} + a, s_i - 1) + 1)   to   min(N, s_i + a, s_{i+1} - 1):
// everything its predecessor's `after` does not reach, up to the line in front of its successor.  The owned ranges are disjoint,
// ascending with i, and their union is the union above; each depends on the two neighbours only.  Additions and subtractions
// saturate, so b and a may be anything up to 2^64 - 1.
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SS_CTX_HD __host__ __device__ inline
#else
#define SS_CTX_HD inline
#endif

namespace ss {

SS_CTX_HD uint64_t ctx_sat_add(uint64_t x, uint64_t y) { return x + y < x ? ~0ull : x + y; }
SS_CTX_HD uint64_t ctx_sat_sub(uint64_t x, uint64_t y) { return x < y ? 0ull : x - y; }

struct CtxRange {
    uint64_t lo, hi;            // lines lo .. hi, both included; lo > hi: none
};
SS_CTX_HD uint64_t ctx_size(const CtxRange &r) { return r.lo > r.hi ? 0ull : r.hi - r.lo + 1; }

// The lines entry `s` owns among 1 .. N.  prev / next: the entries in front of and behind it, 0 where there is none.  An entry of 0
// or above N is invalid: it owns nothing, and as a neighbour it takes nothing away.  A neighbour that is out of order (prev >= s,
// next <= s: the caller broke the contract) is ignored, so every range stays inside [1, N] and holds s whatever the input is.
SS_CTX_HD CtxRange ctx_range(uint64_t prev, uint64_t s, uint64_t next, uint64_t N, uint64_t before, uint64_t after)
{
    CtxRange r = {1, 0};
    if (s == 0 || s > N) return r;
    uint64_t lo = ctx_sat_sub(s, before);
    if (lo < 1) lo = 1;
    if (prev >= 1 && prev < s) {
        uint64_t reach = ctx_sat_add(prev, after);          // the last line the predecessor owns ...
        if (reach > s - 1) reach = s - 1;
        if (reach + 1 > lo) lo = reach + 1;                 // ... and the first one left for this entry
    }
    uint64_t hi = ctx_sat_add(s, after);
    if (hi > N) hi = N;
    if (next > s && next - 1 < hi) hi = next - 1;
    r.lo = lo;
    r.hi = hi;
    return r;
}

}  // namespace ss
