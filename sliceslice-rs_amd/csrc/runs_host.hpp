// runs_host.hpp - the host side of the run patterns (include/sliceslice_hip_runs.h has THE RULE and the language; ss_runs.hip uses
// this file, tests/native/runs_host_check.cpp sweeps it under sanitizers).  Plain C++, no HIP call:
//   parse_runs     ONE item of the classes language (classes_host.hpp's escape and bracket routines, called) and one quantifier
//                  -> the set and (min_len, max_len), or the offending column
//   check_lengths  the bounds of THE RULE
#pragma once
#include "classes_host.hpp"
#include "runs_swar.hpp"

namespace ssh {
namespace runs {

constexpr uint64_t kMaxLen = 4096;          // SS_RUNS_MAX_LEN

// NULL, or what is wrong with (min_len, max_len)
inline const char *check_lengths(uint64_t min_len, uint64_t max_len)
{
    if (min_len == 0) return "min_len is 0: a run holds at least one byte";
    if (min_len > kMaxLen) return "min_len is above 4096 (SS_RUNS_MAX_LEN)";
    if (max_len > kMaxLen) return "max_len is above 4096 (SS_RUNS_MAX_LEN)";
    if (max_len != 0 && max_len < min_len) return "max_len is below min_len";
    return nullptr;
}

// false: refused, *err says where and why, nothing is written.
inline bool parse_runs(const char *text, bool ignore_case, uint64_t *set, uint64_t *min_len, uint64_t *max_len, classes::ParseError *err)
{
    using namespace classes;
    const detail::Text x = {reinterpret_cast<const unsigned char *>(text), std::strlen(text), err};
    size_t i = 0;
    const unsigned c = x.t[0];
    Set s = Set{{0, 0, 0, 0}};
    if (c == 0) return x.fail(0, "an empty text: one item and one of + {k} {k,} {k,m}");
    if (c == '\\') {
        bool is_class;
        unsigned byte;
        if (!detail::escape(x, i, s, is_class, byte)) return false;
        if (ignore_case) detail::close_case(s);
    } else if (c == '[') {
        if (!detail::bracket(x, i, ignore_case, s)) return false;
    } else if (c == '.') {
        s = Set{{~0ull, ~0ull, ~0ull, ~0ull}};
        ++i;
    } else if (std::strchr("](){}*+?|^$", (int)c) != nullptr) {
        return x.fail(0, "one of ] } ( ) { * + ? | ^ $ in place of the item: no groups, alternatives or anchors");
    } else {
        set_add(s, c);
        if (ignore_case) detail::close_case(s);
        ++i;
    }
    uint64_t lo = 0, hi = 0;
    const unsigned q = x.t[i];
    if (q == '+') {
        lo = 1;
        ++i;
    } else if (q == '*' || q == '?') {
        return x.fail(i, "* and ? would match the empty string: a run holds at least one byte");
    } else if (q == '{') {
        auto number = [&](size_t &j, uint64_t &v) {
            size_t digits = 0;
            for (v = 0; x.t[j] >= '0' && x.t[j] <= '9'; ++j, ++digits) v = v > kMaxLen ? v : v * 10 + (x.t[j] - '0');
            return digits;
        };
        size_t j = i + 1;
        const size_t kat = j;
        if (x.t[j] == ',') return x.fail(j, "{,m} would match the empty string: a run holds at least one byte");
        if (number(j, lo) == 0) return x.fail(j, "a repetition is {k}, {k,} or {k,m}");
        if (lo == 0) return x.fail(kat, "{0...} would match the empty string: a run holds at least one byte");
        if (lo > kMaxLen) return x.fail(kat, "a repetition count is 1 .. 4096");
        if (x.t[j] == '}') {
            hi = lo;
        } else if (x.t[j] == ',') {
            ++j;
            const size_t mat = j;
            if (x.t[j] != '}') {
                if (number(j, hi) == 0 || x.t[j] != '}') return x.fail(j, "a repetition is {k}, {k,} or {k,m}");
                if (hi > kMaxLen) return x.fail(mat, "a repetition count is 1 .. 4096");
                if (hi < lo) return x.fail(mat, "{k,m} with m < k");
            }
        } else {
            return x.fail(j, "a repetition is {k}, {k,} or {k,m}");
        }
        i = j + 1;
    } else {
        return x.fail(i, "the item is not followed by one of + {k} {k,} {k,m}");
    }
    if (x.t[i] != 0) return x.fail(i, "something behind the quantifier: a run pattern is ONE item and ONE quantifier");
    if (set) std::memcpy(set, s.w, sizeof s.w);
    if (min_len) *min_len = lo;
    if (max_len) *max_len = hi;
    return true;
}

}  // namespace runs
}  // namespace ssh
