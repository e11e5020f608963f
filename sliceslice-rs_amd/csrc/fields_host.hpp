// fields_host.hpp - the host side of the field selections (include/sliceslice_hip_fields.h has THE RULE and the language;
// ss_fields.hip uses this file).  Plain C++, no HIP call:
//   parse_fields      cut's single range K, K-, K-M, -M -> (first, last), or the offending column
//   check_selection   the bounds of THE RULE
#pragma once
#include <cstddef>
#include <cstdint>

namespace ssh {
namespace fields {

struct ParseError {
    size_t column;          // from 1
    const char *what;
};

// NULL, or what is wrong with (mode, first, last, flags)
inline const char *check_selection(int mode, uint64_t first, uint64_t last, unsigned flags)
{
    if (mode != 0 && mode != 1) return "the mode is neither SS_FIELDS_EACH (0) nor SS_FIELDS_MERGE (1)";
    if (flags & ~1u) return "unknown flag bits (SS_FIELDS_KEEP_SHORT is the only flag)";
    if (first == 0) return "first is 0: fields are numbered from 1";
    if (last != 0 && last < first) return "last is below first";
    return nullptr;
}

// false: refused, *err says where and why, nothing is written.
inline bool parse_fields(const char *text, uint64_t *first, uint64_t *last, ParseError *err)
{
    auto fail = [&](size_t at, const char *what) {
        err->column = at + 1;
        err->what = what;
        return false;
    };
    // a decimal number at text[i]: 0 digits -> *digits == 0
    auto number = [&](size_t &i, uint64_t &v, size_t &digits, bool &overflow) {
        v = 0;
        digits = 0;
        overflow = false;
        for (; text[i] >= '0' && text[i] <= '9'; ++i, ++digits) {
            const uint64_t d = (uint64_t)(text[i] - '0');
            if (v > (UINT64_MAX - d) / 10) overflow = true;
            else v = v * 10 + d;
        }
    };
    if (text[0] == 0) return fail(0, "an empty text: a range is K, K-, K-M or -M");
    size_t i = 0, digits = 0;
    uint64_t lo = 1, hi = 0;
    bool over = false;
    if (text[i] != '-') {
        const size_t at = i;
        number(i, lo, digits, over);
        if (digits == 0) return fail(at, text[at] == ',' ? "a comma list: make one call per range" : "a range is K, K-, K-M or -M, in decimal digits");
        if (over) return fail(at, "a field number that does not fit 64 bits");
        if (lo == 0) return fail(at, "field 0: fields are numbered from 1");
        hi = lo;
    }
    if (text[i] == '-') {
        ++i;
        const size_t at = i;
        number(i, hi, digits, over);
        if (digits == 0) {
            if (at == 1 && text[0] == '-') return fail(at, text[at] == ',' ? "a comma list: make one call per range" : "- without a number: a range is K, K-, K-M or -M");
            hi = 0;                                                             // K-
        } else {
            if (over) return fail(at, "a field number that does not fit 64 bits");
            if (hi == 0) return fail(at, "field 0: fields are numbered from 1");
            if (hi < lo) return fail(at, "K-M with M < K");
        }
    }
    if (text[i] == ',') return fail(i, "a comma list: make one call per range");
    if (text[i] != 0) return fail(i, "a range is K, K-, K-M or -M, in decimal digits");
    *first = lo;
    *last = hi;
    return true;
}

}  // namespace fields
}  // namespace ssh
