// output_host.hpp - the arithmetic of the output rule (include/sliceslice_hip_output.h): how many digits a number has, which byte
// stands at a position of its decimal form, the clamp of a record to the view, whether a separator stands in front of a record, and
// the bytes a record contributes.  Free of HIP, so that a stand-alone program can sweep it (tests/native/output_host_check.cpp); the
// kernels (output_kernels.hpp) compile the same functions for the device by defining SS_OUTPUT_FN before they include this file.
// Nothing here is exported.
#pragma once
#include <cstddef>
#include <cstdint>

#ifndef SS_OUTPUT_FN
#define SS_OUTPUT_FN inline
#endif

namespace ss {

constexpr unsigned kOutNumber = 1u, kOutSeparator = 2u;         // SS_OUTPUT_NUMBER, SS_OUTPUT_SEPARATOR

// 10^k, k = 0 .. 19
SS_OUTPUT_FN uint64_t out_pow10(int k)
{
    uint64_t p = 1;
    for (int j = 0; j < k; ++j) p *= 10u;
    return p;
}

// the decimal digits of v: 1 .. 20, no leading zeros, 0 has one
SS_OUTPUT_FN int out_digits(uint64_t v)
{
    int n = 1;
    uint64_t p = 10u;
    while (n < 20 && v >= p) {
        ++n;
        p *= 10u;                                               // (10^20 is never formed: the loop ends at n == 20)
    }
    return n;
}

// digit `pos` (0: the most significant) of the `digits`-digit number v, as its ASCII byte
SS_OUTPUT_FN uint8_t out_digit(uint64_t v, int digits, int pos)
{
    return (uint8_t)('0' + (v / out_pow10(digits - 1 - pos)) % 10u);
}

// v in decimal into dst[0, out_digits(v)); returns the number of bytes
SS_OUTPUT_FN int out_write_decimal(uint64_t v, uint8_t *dst)
{
    const int n = out_digits(v);
    for (int k = 0; k < n; ++k) dst[k] = out_digit(v, n, k);
    return n;
}

// the record's bytes of the view: e = min(end, len), b = min(begin, e)
SS_OUTPUT_FN void out_clamp(uint64_t begin, uint64_t end, uint64_t len, uint64_t *b, uint64_t *e)
{
    *e = end < len ? end : len;
    *b = begin < *e ? begin : *e;
}

// number[i] > number[i-1] + 1, without wrapping
SS_OUTPUT_FN bool out_separated(uint64_t prev, uint64_t cur) { return cur > prev && cur - prev > 1u; }

// What stands in front of a record's text: the separator's bytes (0, 2 or 3) and the number's (digits and `:` / `-`, or 0).
// `first`: the record has no predecessor.
struct OutPrefix {
    uint32_t sep, num;
};
SS_OUTPUT_FN OutPrefix out_prefix(unsigned flags, int terminator, bool first, uint64_t prev, uint64_t number)
{
    OutPrefix p;
    p.sep = (flags & kOutSeparator) && !first && out_separated(prev, number) ? 2u + (terminator >= 0 ? 1u : 0u) : 0u;
    p.num = (flags & kOutNumber) ? (uint32_t)out_digits(number) + 1u : 0u;
    return p;
}

// the bytes record i contributes
SS_OUTPUT_FN uint64_t out_record_size(unsigned flags, int terminator, bool first, uint64_t prev, uint64_t number, uint64_t begin, uint64_t end,
                                      uint64_t len)
{
    uint64_t b, e;
    out_clamp(begin, end, len, &b, &e);
    const OutPrefix p = out_prefix(flags, terminator, first, prev, number);
    return (uint64_t)p.sep + p.num + (e - b) + (terminator >= 0 ? 1u : 0u);
}

}  // namespace ss
