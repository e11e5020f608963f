// classes_host.hpp - the host side of the byte-class patterns (include/sliceslice_hip_classes.h has THE RULE and the pattern language;
// ss_classes.hip uses this file, tests/native/classes_host_check.cpp sweeps it under sanitizers).  Plain C++, no HIP call:
//   parse_classes      the pattern language -> one set of 256 bits per position, or the offending column
//   class_cover        the tightest (value, mask) pair of a set
//   make_class_plan    covers of every position, the split into single / masked / inexact positions, the distinct inexact sets and
//                      the check list, rarest set first
//   choose_class_filter  ss_masked_choose_filter's rule on the covers (the existing routine, called, not restated)
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/sliceslice_hip_masked.h"

namespace ssh {
namespace classes {

constexpr size_t kMaxLen = 4096;            // SS_CLASSES_MAX_LEN
constexpr size_t kMaxInexact = 1024;        // SS_CLASSES_MAX_INEXACT
constexpr size_t kMaxDistinct = 64;         // SS_CLASSES_MAX_DISTINCT

struct Set {
    uint64_t w[4];
};

inline bool set_has(const uint64_t *w, unsigned b) { return (w[b >> 6] >> (b & 63)) & 1u; }
inline void set_add(Set &s, unsigned b) { s.w[b >> 6] |= 1ull << (b & 63); }
inline void set_add_range(Set &s, unsigned lo, unsigned hi)
{
    for (unsigned b = lo; b <= hi; ++b) set_add(s, b);
}
inline void set_or(Set &s, const Set &o)
{
    for (int k = 0; k < 4; ++k) s.w[k] |= o.w[k];
}
inline unsigned set_size(const uint64_t *w)
{
    return (unsigned)(__builtin_popcountll(w[0]) + __builtin_popcountll(w[1]) + __builtin_popcountll(w[2]) + __builtin_popcountll(w[3]));
}
inline bool set_equal(const uint64_t *a, const uint64_t *b) { return a[0] == b[0] && a[1] == b[1] && a[2] == b[2] && a[3] == b[3]; }

// ---- the parser ---------------------------------------------------------------------------------------------------------------------
// What was refused: the column (from 1, always inside the text; 1 for an empty text) and why.
struct ParseError {
    size_t column;
    const char *what;
};

namespace detail {

struct Text {
    const unsigned char *t;
    size_t len;
    ParseError *err;
    bool fail(size_t at, const char *what) const
    {
        err->column = len == 0 ? 1 : (at < len ? at : len - 1) + 1;
        err->what = what;
        return false;
    }
};

inline int hex_digit(unsigned c)
{
    if (c >= '0' && c <= '9') return (int)(c - '0');
    if (c >= 'a' && c <= 'f') return (int)(c - 'a' + 10);
    if (c >= 'A' && c <= 'F') return (int)(c - 'A' + 10);
    return -1;
}

inline bool ascii_punctuation(unsigned c) { return (c >= 0x21 && c <= 0x2F) || (c >= 0x3A && c <= 0x40) || (c >= 0x5B && c <= 0x60) || (c >= 0x7B && c <= 0x7E); }

// t[i] is a backslash: the escape's set, whether it is a class escape, and i behind it
inline bool escape(const Text &x, size_t &i, Set &out, bool &is_class, unsigned &byte)
{
    const unsigned c = x.t[i + 1];
    out = Set{{0, 0, 0, 0}};
    is_class = false;
    byte = 0;
    if (c == 0) return x.fail(i, "the text ends inside an escape");
    Set word = Set{{0, 0, 0, 0}}, digit = Set{{0, 0, 0, 0}}, space = Set{{0, 0, 0, 0}};
    set_add_range(digit, '0', '9');
    set_add_range(word, '0', '9');
    set_add_range(word, 'A', 'Z');
    set_add_range(word, 'a', 'z');
    set_add(word, '_');
    set_add_range(space, 9, 13);
    set_add(space, ' ');
    const Set *cls = nullptr;
    switch (c) {
    case 'd': case 'D': cls = &digit; break;
    case 'w': case 'W': cls = &word; break;
    case 's': case 'S': cls = &space; break;
    case 'n': byte = '\n'; break;
    case 't': byte = '\t'; break;
    case 'r': byte = '\r'; break;
    case 'f': byte = '\f'; break;
    case 'v': byte = '\v'; break;
    case 'x': {
        const int hi = hex_digit(x.t[i + 2]);
        if (hi < 0) return x.fail(i + 2, "\\x takes exactly two hex digits");
        const int lo = hex_digit(x.t[i + 3]);
        if (lo < 0) return x.fail(i + 3, "\\x takes exactly two hex digits");
        byte = (unsigned)(hi * 16 + lo);
        i += 2;
        break;
    }
    default:
        if (!ascii_punctuation(c)) return x.fail(i + 1, "an escape is one of \\d \\D \\w \\W \\s \\S \\n \\t \\r \\f \\v \\xHH or a backslash before ASCII punctuation");
        byte = c;
    }
    i += 2;
    if (cls) {
        is_class = true;
        out = *cls;
        if (c == 'D' || c == 'W' || c == 'S')
            for (int k = 0; k < 4; ++k) out.w[k] = ~out.w[k];
    } else {
        set_add(out, byte);
    }
    return true;
}

// closed under swapping ASCII case
inline void close_case(Set &s)
{
    for (unsigned b = 'A'; b <= 'Z'; ++b) {
        if (set_has(s.w, b) || set_has(s.w, b | 0x20u)) {
            set_add(s, b);
            set_add(s, b | 0x20u);
        }
    }
}

// t[i] is '[': the set and i behind its ']'
inline bool bracket(const Text &x, size_t &i, bool ignore_case, Set &out)
{
    const size_t open = i;
    size_t j = i + 1;
    const bool negate = x.t[j] == '^';
    if (negate) ++j;
    Set pos = Set{{0, 0, 0, 0}};
    for (bool first = true;; first = false) {
        const unsigned c = x.t[j];
        if (c == 0) return x.fail(open, "a set is not closed by ]");
        if (c == ']') {
            if (first) return x.fail(j, "a ] in first place of a set");
            break;
        }
        if (c == '[') return x.fail(j, "an unescaped [ inside a set");
        const size_t xat = j;
        Set xs = Set{{0, 0, 0, 0}};
        bool xclass = false;
        unsigned xb = 0;
        if (c == '\\') {
            if (!escape(x, j, xs, xclass, xb)) return false;
        } else {
            if ((c == '-' || c == '&' || c == '~' || c == '|') && x.t[j + 1] == c) return x.fail(j + 1, "a doubled -- && ~~ || inside a set");
            if (c == '-' && !first && x.t[j + 1] != ']')
                return x.fail(j, "a - inside a set is a literal only directly after the opening or directly before ]");
            xb = c;
            set_add(xs, xb);
            ++j;
        }
        if (x.t[j] == '-' && x.t[j + 1] != ']') {                       // a range x-y
            const size_t yat = j + 1;
            const unsigned y = x.t[yat];
            if (y == 0) return x.fail(open, "a set is not closed by ]");
            if (y == '-') return x.fail(yat, "a doubled -- && ~~ || inside a set");
            if (y == '[') return x.fail(yat, "an unescaped [ inside a set");
            Set ys = Set{{0, 0, 0, 0}};
            bool yclass = false;
            unsigned yb = y;
            j = yat;
            if (y == '\\') {
                if (!escape(x, j, ys, yclass, yb)) return false;
            } else {
                ++j;
            }
            if (xclass) return x.fail(xat, "a range with a class escape as an end");
            if (yclass) return x.fail(yat, "a range with a class escape as an end");
            if (xb > yb) return x.fail(xat, "a reversed range");
            set_add_range(pos, xb, yb);
        } else {
            set_or(pos, xs);
        }
    }
    if (ignore_case) close_case(pos);
    if (negate)
        for (int k = 0; k < 4; ++k) pos.w[k] = ~pos.w[k];
    if (set_size(pos.w) == 0) return x.fail(open, "a set that accepts no byte");
    out = pos;
    i = j + 1;
    return true;
}

}  // namespace detail

// The pattern language of include/sliceslice_hip_classes.h.  The sets of the positions k < capacity go to `sets` (4 words each; may
// be NULL) and *n is the number of positions.  false: refused, *err says where and why, *n is untouched.
inline bool parse_classes(const char *text, bool ignore_case, uint64_t *sets, size_t capacity, size_t *n, ParseError *err)
{
    const detail::Text x = {reinterpret_cast<const unsigned char *>(text), std::strlen(text), err};
    size_t count = 0, i = 0;
    bool have_item = false;                 // the byte in front closed an item that may be repeated
    Set last = Set{{0, 0, 0, 0}};
    auto emit = [&](const Set &s, size_t copies, size_t at) {
        if (copies > kMaxLen - count) return x.fail(at, "more than 4096 positions");
        for (size_t k = 0; k < copies; ++k, ++count)
            if (sets && count < capacity) std::memcpy(sets + 4 * count, s.w, sizeof s.w);
        return true;
    };
    while (x.t[i] != 0) {
        const unsigned c = x.t[i];
        const size_t at = i;
        if (c == '{') {
            if (!have_item) return x.fail(i, "a { that does not follow an item");
            size_t j = i + 1, k = 0, digits = 0;
            for (; x.t[j] >= '0' && x.t[j] <= '9'; ++j, ++digits) k = k > kMaxLen ? k : k * 10 + (x.t[j] - '0');
            if (digits == 0 || x.t[j] != '}') return x.fail(j, "a repetition is {k} with one number");
            if (k == 0 || k > kMaxLen) return x.fail(i + 1, "a repetition count is 1 .. 4096");
            if (!emit(last, k - 1, at)) return false;
            have_item = false;
            i = j + 1;
            continue;
        }
        Set s = Set{{0, 0, 0, 0}};
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
            return x.fail(i, "one of ] } ( ) * + ? | ^ $ outside a set: no groups, variable lengths, alternatives or anchors");
        } else {
            set_add(s, c);
            if (ignore_case) detail::close_case(s);
            ++i;
        }
        if (!emit(s, 1, at)) return false;
        last = s;
        have_item = true;
    }
    *n = count;
    return true;
}

// ---- the cover ----------------------------------------------------------------------------------------------------------------------
// The tightest (value, mask) of a non-empty set: mask = ~(OR over members c of c ^ c0), value = c0 & mask.
inline void class_cover(const uint64_t *set, uint8_t *value, uint8_t *mask)
{
    unsigned c0 = 256, diff = 0;
    for (unsigned b = 0; b < 256; ++b) {
        if (!set_has(set, b)) continue;
        if (c0 == 256) c0 = b;
        diff |= b ^ c0;
    }
    *mask = (uint8_t)~diff;
    *value = (uint8_t)(c0 & ~diff);
}

// the number of byte values (value, mask) accepts
inline unsigned cover_size(uint8_t mask) { return 1u << __builtin_popcount((unsigned)(uint8_t)~mask); }

// ---- the plan -----------------------------------------------------------------------------------------------------------------------
struct Plan {
    std::vector<uint8_t> value, mask;       // the cover of every position
    std::vector<uint64_t> bitmaps;          // the distinct inexact sets in the order of their first position, 4 words each
    std::vector<uint32_t> checks;           // one entry per inexact position, position | set id << 16, rarest set first
    uint64_t single = 0, masked = 0, inexact = 0;
};

enum PlanResult { kPlanOk = 0, kPlanEmptySet, kPlanTooManyInexact, kPlanTooManyDistinct };

// `cost`: the static cost of every byte value (the table the filter choice uses).  On kPlanEmptySet *where is the position.
inline PlanResult make_class_plan(const uint64_t *sets, size_t n, const int *cost, Plan *plan, size_t *where)
{
    *plan = Plan();
    plan->value.resize(n);
    plan->mask.resize(n);
    std::vector<uint64_t> set_cost;
    for (size_t i = 0; i < n; ++i) {
        const uint64_t *s = sets + 4 * i;
        const unsigned members = set_size(s);
        if (members == 0) {
            *where = i;
            return kPlanEmptySet;
        }
        class_cover(s, &plan->value[i], &plan->mask[i]);
        if (members == 1) {
            ++plan->single;
        } else if (members == cover_size(plan->mask[i])) {
            ++plan->masked;
        } else {
            if (++plan->inexact > kMaxInexact) return kPlanTooManyInexact;
            size_t id = 0;
            const size_t distinct = plan->bitmaps.size() / 4;
            while (id < distinct && !set_equal(&plan->bitmaps[4 * id], s)) ++id;
            if (id == distinct) {
                if (distinct == kMaxDistinct) return kPlanTooManyDistinct;
                plan->bitmaps.insert(plan->bitmaps.end(), s, s + 4);
                uint64_t sum = 0;
                for (unsigned b = 0; b < 256; ++b)
                    if (set_has(s, b)) sum += (uint64_t)cost[b];
                set_cost.push_back(sum);
            }
            plan->checks.push_back((uint32_t)i | (uint32_t)id << 16);
        }
    }
    std::stable_sort(plan->checks.begin(), plan->checks.end(),
                     [&](uint32_t a, uint32_t b) { return set_cost[a >> 16] < set_cost[b >> 16]; });      // (ties stay in position order)
    return kPlanOk;
}

// ss_masked_choose_filter on the covers: the register test lets through what the COVER accepts, so that is what is costed.
inline int choose_class_filter(const Plan &plan, size_t *anchor, size_t *distance)
{
    return ss_masked_choose_filter(plan.value.data(), plan.mask.data(), plan.value.size(), nullptr, anchor, distance);
}

}  // namespace classes
}  // namespace ssh
