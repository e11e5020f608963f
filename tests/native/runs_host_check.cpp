// runs_host_check.cpp - the host side of the run patterns in a program of its own (tests/test_runs_cpu.py builds it with
// -fsanitize=address,undefined and runs it): runs_swar.hpp's range test against the plain comparison for EVERY (lo, hi) with
// lo <= hi and every byte value in every lane of the dword; runs_ranges on the sets the header names and on sets of 1, 4, 5 and 128
// ranges; runs_host.hpp's parser on what it accepts and on every refusal, with the column.
#include "../../sliceslice-rs_amd/csrc/runs_host.hpp"

#include <cstdio>

static long checks = 0, failures = 0;

static void expect(bool ok, const char *what, long a = 0, long b = 0, long c = 0)
{
    ++checks;
    if (!ok) {
        ++failures;
        if (failures < 20) std::printf("FAILED %s (%ld, %ld, %ld)\n", what, a, b, c);
    }
}

static void sweep_swar()
{
    for (unsigned lo = 0; lo < 256; ++lo) {
        for (unsigned hi = lo; hi < 256; ++hi) {
            const ss::RunsRange r = ss::runs_range(lo, hi);
            for (unsigned b = 0; b < 256; ++b) {
                const bool want = b >= lo && b <= hi;
                // the byte in every lane, its neighbours first all zero, then all ones, then a pattern that would carry
                const uint32_t fills[3] = {0x00000000u, 0xFFFFFFFFu, 0x7F80FF01u};
                for (int lane = 0; lane < 4; ++lane) {
                    for (uint32_t fill : fills) {
                        const uint32_t x = (fill & ~(0xFFu << (8 * lane))) | (b << (8 * lane));
                        const uint32_t z = ss::runs_in_range4(x, r);
                        expect(((z >> (8 * lane + 7)) & 1u) == (want ? 1u : 0u), "range test", lo, hi, b);
                        expect((z & 0x7F7F7F7Fu) == 0, "only bit 7 of a byte is set", lo, hi, b);
                        for (int other = 0; other < 4; ++other) {
                            const unsigned ob = (x >> (8 * other)) & 0xFFu;
                            if (((z >> (8 * other + 7)) & 1u) != ((ob >= lo && ob <= hi) ? 1u : 0u)) expect(false, "a neighbouring lane", lo, hi, ob);
                        }
                    }
                }
            }
        }
    }
}

static void set_range(uint64_t *s, unsigned lo, unsigned hi)
{
    for (unsigned b = lo; b <= hi; ++b) s[b >> 6] |= 1ull << (b & 63);
}

static unsigned ranges_of(const uint64_t *s, uint8_t *lo, uint8_t *hi) { return ss::runs_ranges(s, lo, hi, 4); }

static void sweep_ranges()
{
    uint8_t lo[4], hi[4];
    {
        uint64_t w[4] = {0, 0, 0, 0};                               // \w
        set_range(w, '0', '9'), set_range(w, 'A', 'Z'), set_range(w, 'a', 'z'), set_range(w, '_', '_');
        expect(ranges_of(w, lo, hi) == 4 && lo[0] == '0' && hi[0] == '9' && lo[1] == 'A' && hi[1] == 'Z' && lo[2] == '_' && hi[2] == '_' &&
                   lo[3] == 'a' && hi[3] == 'z', "\\w has 4 ranges");
    }
    {
        uint64_t w[4] = {~0ull, ~0ull, ~0ull, ~0ull};               // \S: everything but 9 .. 13 and the blank
        for (unsigned b : {9u, 10u, 11u, 12u, 13u, 32u}) w[b >> 6] &= ~(1ull << (b & 63));
        expect(ranges_of(w, lo, hi) == 3 && lo[0] == 0 && hi[0] == 8 && lo[1] == 14 && hi[1] == 31 && lo[2] == 33 && hi[2] == 255, "\\S has 3 ranges");
    }
    {
        uint64_t w[4] = {0, 0, 0, 0};                               // [0-9A-Fa-f]
        set_range(w, '0', '9'), set_range(w, 'A', 'F'), set_range(w, 'a', 'f');
        expect(ranges_of(w, lo, hi) == 3, "[0-9A-Fa-f] has 3 ranges");
    }
    {
        uint64_t w[4] = {~0ull, ~0ull, ~0ull, ~0ull};               // [^\n]
        w[0] &= ~(1ull << 10);
        expect(ranges_of(w, lo, hi) == 2 && lo[0] == 0 && hi[0] == 9 && lo[1] == 11 && hi[1] == 255, "[^\\n] has 2 ranges");
    }
    {
        uint64_t w[4] = {~0ull, ~0ull, ~0ull, ~0ull};               // the full set
        expect(ranges_of(w, lo, hi) == 1 && lo[0] == 0 && hi[0] == 255, "the full set is 1 range");
        uint64_t one[4] = {0, 0, 0, 1ull << 63};
        expect(ranges_of(one, lo, hi) == 1 && lo[0] == 255 && hi[0] == 255, "0xFF alone is 1 range");
        uint64_t none[4] = {0, 0, 0, 0};
        expect(ranges_of(none, lo, hi) == 0, "the empty set has none");
    }
    {
        uint64_t w[4] = {0, 0, 0, 0};                               // 5 ranges: the first four are written, the count is 5
        for (unsigned k = 0; k < 5; ++k) set_range(w, 40 * k, 40 * k + 7);
        lo[3] = hi[3] = 0;
        expect(ranges_of(w, lo, hi) == 5 && lo[3] == 120 && hi[3] == 127, "5 ranges");
        uint64_t x[4] = {0, 0, 0, 0};
        for (unsigned k = 0; k < 4; ++k) set_range(x, 63 * k + 1, 63 * k + 64);     // ranges that cross the words
        expect(ranges_of(x, lo, hi) == 1 && lo[0] == 1 && hi[0] == 253, "adjacent ranges join across the words");
    }
    {
        const uint64_t odd = 0xAAAAAAAAAAAAAAAAull;                 // every odd value: 128 ranges
        uint64_t w[4] = {odd, odd, odd, odd};
        expect(ranges_of(w, lo, hi) == 128 && lo[0] == 1 && hi[0] == 1 && lo[3] == 7, "128 ranges");
    }
}

struct Accepted {
    const char *text;
    uint64_t lo, hi;
};
struct Refused {
    const char *text;
    size_t column;
};

static void sweep_parser()
{
    using namespace ssh;
    const Accepted good[] = {{"a+", 1, 0}, {"\\w+", 1, 0}, {"[0-9]{3,}", 3, 0}, {"[A-Z]{2,5}", 2, 5}, {" {2,}", 2, 0}, {"[^\\n]{80,}", 80, 0},
                             {".{7}", 7, 7}, {"\\x41{4096}", 4096, 4096}, {"a{1,4096}", 1, 4096}, {"a{4096,}", 4096, 0}, {"[+]+", 1, 0},
                             {"\\++", 1, 0}, {"a{3,3}", 3, 3}, {"a{007}", 7, 7}};
    for (const Accepted &g : good) {
        uint64_t set[4] = {0, 0, 0, 0}, lo = 77, hi = 77;
        classes::ParseError err = {0, nullptr};
        expect(runs::parse_runs(g.text, false, set, &lo, &hi, &err) && lo == g.lo && hi == g.hi && classes::set_size(set) != 0, g.text);
        expect(runs::check_lengths(lo, hi) == nullptr, g.text);
    }
    const Refused bad[] = {{"", 1}, {"a", 1}, {"\\w", 2}, {"[0-9]", 5}, {"a*", 2}, {"a?", 2}, {"\\w*", 3}, {"a{0}", 3}, {"a{0,}", 3}, {"a{0,5}", 3},
                           {"a{,5}", 3}, {"a+b", 3}, {"a++", 3}, {"a+?", 3}, {"a{2}{3}", 5}, {"ab+", 2}, {"a{4097}", 3}, {"a{2,4097}", 5},
                           {"a{99999999999999999999,}", 3}, {"a{5,2}", 5}, {"a{}", 3}, {"a{2", 3}, {"a{2,", 4}, {"a{2,x}", 5}, {"a{x}", 3}, {"a{2,3", 5},
                           {"+", 1}, {"*", 1}, {"{2}", 1}, {"(a)+", 1}, {"^a+", 1}, {"a|b", 2}, {"[a", 1}, {"[]+", 2}, {"\\q+", 2}, {"[z-a]+", 2},
                           {"\\w+$", 4}, {"a{3,5}x", 7}};
    for (const Refused &b : bad) {
        uint64_t set[4] = {5, 5, 5, 5}, lo = 77, hi = 77;
        classes::ParseError err = {0, nullptr};
        const bool ok = runs::parse_runs(b.text, false, set, &lo, &hi, &err);
        expect(!ok && err.column == b.column && err.what != nullptr, b.text, (long)err.column, (long)b.column);
        expect(set[0] == 5 && set[3] == 5 && lo == 77 && hi == 77, "a refusal writes nothing");
        classes::ParseError err2 = {0, nullptr};
        expect(!runs::parse_runs(b.text, true, set, &lo, &hi, &err2) && err2.column == b.column, b.text);
    }
    expect(runs::check_lengths(0, 0) != nullptr && runs::check_lengths(4097, 0) != nullptr && runs::check_lengths(1, 4097) != nullptr &&
               runs::check_lengths(5, 4) != nullptr && runs::check_lengths(4096, 4096) == nullptr && runs::check_lengths(1, 0) == nullptr,
           "the bounds of the rule");
    // ignore_case closes the positive set, then negates
    uint64_t set[4], lo, hi;
    classes::ParseError err = {0, nullptr};
    expect(runs::parse_runs("[a-c]+", true, set, &lo, &hi, &err) && classes::set_has(set, 'B') && classes::set_size(set) == 6, "[a-c]+ with -i");
    expect(runs::parse_runs("[^a]+", true, set, &lo, &hi, &err) && !classes::set_has(set, 'A') && classes::set_size(set) == 254, "[^a]+ with -i");
}

int main()
{
    sweep_swar();
    sweep_ranges();
    sweep_parser();
    std::printf("runs_host_check: %ld checks %ld failures\n", checks, failures);
    return failures == 0 ? 0 : 1;
}
