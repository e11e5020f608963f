// classes_host_check.cpp - a sweep of sliceslice-rs_amd/csrc/classes_host.hpp against loops written out, compiled for the host alone
// (tests/test_classes_cpu.py builds it with -fsanitize=address,undefined and runs it as a child):
//   * parse_classes on every text up to length 4 over the alphabet a [ ] ^ - \ d { 2 } . with and without ignore_case, into an
//     array of exactly `capacity` sets: no crash, no write behind the capacity, and a refusal's column is inside the text; the
//     counting call (NULL sets) and the writing call agree;
//   * class_cover against the definition written out, for 2,000 random sets: every member passes, and no mask with one more bit
//     does for any value;
//   * make_class_plan against a classification written out: single / masked / inexact counts, the distinct sets in order of first
//     appearance, the check list ascending by summed cost with ties by position, and the two limits at their edges.
// Prints "<checks> checks, <failures> failures" and exits with the number of failures (capped).
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../sliceslice-rs_amd/csrc/classes_host.hpp"

using namespace ssh::classes;

static long checks = 0, failures = 0;

static void expect(bool ok, const char *what, const std::string &detail = "")
{
    ++checks;
    if (!ok && ++failures <= 20) std::printf("FAILED %s %s\n", what, detail.c_str());
}

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd()
{
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return rng_state;
}

static void sweep_parser()
{
    const char alphabet[] = "a[]^-\\d{2}.";
    const int k = (int)std::strlen(alphabet);
    for (int len = 0; len <= 4; ++len) {
        long total = 1;
        for (int i = 0; i < len; ++i) total *= k;
        for (long code = 0; code < total; ++code) {
            std::string text;
            long c = code;
            for (int i = 0; i < len; ++i, c /= k) text += alphabet[c % k];
            for (int ic = 0; ic < 2; ++ic) {
                size_t n = 9999;
                ParseError err = {0, nullptr};
                const bool ok = parse_classes(text.c_str(), ic != 0, nullptr, 0, &n, &err);
                if (!ok) {
                    expect(err.column >= 1 && err.column <= (text.empty() ? 1 : text.size()) && err.what != nullptr && n == 9999, "column", text);
                    continue;
                }
                expect(n <= 4 || text.find('{') != std::string::npos, "positions", text);
                for (size_t capacity : {(size_t)0, (size_t)1, n}) {
                    std::vector<uint64_t> exact(4 * capacity);              // (ASan guards the end)
                    size_t n2 = 0;
                    expect(parse_classes(text.c_str(), ic != 0, exact.data(), capacity, &n2, &err) && n2 == n, "second call", text);
                    for (size_t p = 0; p < capacity && p < n; ++p) expect(set_size(&exact[4 * p]) != 0, "empty set accepted", text);
                }
            }
        }
    }
}

static void sweep_cover()
{
    for (int trial = 0; trial < 2000; ++trial) {
        uint64_t s[4] = {0, 0, 0, 0};
        const int members = 1 + (int)(rnd() % (trial % 2 ? 6 : 200));
        const unsigned spread = (unsigned)(rnd() & 0xFF), base = (unsigned)(rnd() & 0xFF);
        for (int m = 0; m < members; ++m) {
            const unsigned b = trial % 3 == 0 ? (unsigned)(rnd() & 0xFF) : (base ^ ((unsigned)rnd() & spread));
            s[b >> 6] |= 1ull << (b & 63);
        }
        uint8_t value, mask;
        class_cover(s, &value, &mask);
        bool all = true;
        for (unsigned b = 0; b < 256; ++b)
            if (set_has(s, b) && (b & mask) != value) all = false;
        expect(all && (value & ~mask) == 0, "cover accepts every member");
        for (int bit = 0; bit < 8; ++bit) {                                 // one more mask bit loses a member, whatever the value
            if (mask & (1u << bit)) continue;
            bool zero = false, one = false;
            for (unsigned b = 0; b < 256; ++b)
                if (set_has(s, b)) ((b >> bit) & 1u ? one : zero) = true;
            expect(zero && one, "cover is the tightest");
        }
    }
}

static void sweep_plan()
{
    int cost[256];
    for (int b = 0; b < 256; ++b) cost[b] = (b * 37) % 11;
    for (int trial = 0; trial < 400; ++trial) {
        const size_t n = 1 + (size_t)(rnd() % 40);
        std::vector<uint64_t> sets(4 * n, 0);
        std::vector<Set> pool(1 + rnd() % 5);
        for (Set &p : pool) {
            p = Set{{0, 0, 0, 0}};
            for (int m = 1 + (int)(rnd() % 5); m > 0; --m) set_add(p, (unsigned)(rnd() & 0xFF));
        }
        for (size_t i = 0; i < n; ++i) std::memcpy(&sets[4 * i], pool[rnd() % pool.size()].w, 32);
        Plan plan;
        size_t where = 0;
        expect(make_class_plan(sets.data(), n, cost, &plan, &where) == kPlanOk, "plan");
        uint64_t single = 0, masked = 0;
        std::vector<std::vector<uint64_t>> distinct;
        std::vector<uint32_t> inexact_positions;
        for (size_t i = 0; i < n; ++i) {
            const uint64_t *s = &sets[4 * i];
            unsigned members = 0, accepted = 0;
            for (unsigned b = 0; b < 256; ++b) {
                members += set_has(s, b);
                accepted += (b & plan.mask[i]) == plan.value[i];
            }
            if (members == 1) ++single;
            else if (members == accepted) ++masked;
            else {
                inexact_positions.push_back((uint32_t)i);
                std::vector<uint64_t> v(s, s + 4);
                bool seen = false;
                for (const auto &d : distinct) seen = seen || d == v;
                if (!seen) distinct.push_back(v);
            }
        }
        expect(plan.single == single && plan.masked == masked && plan.inexact == inexact_positions.size(), "split");
        expect(plan.bitmaps.size() == 4 * distinct.size() && plan.checks.size() == inexact_positions.size(), "sizes");
        for (size_t d = 0; d < distinct.size() && 4 * d < plan.bitmaps.size(); ++d)
            expect(std::memcmp(&plan.bitmaps[4 * d], distinct[d].data(), 32) == 0, "distinct order");
        std::vector<bool> listed(n, false);
        uint64_t before_cost = 0;
        uint32_t before_position = 0;
        for (size_t k = 0; k < plan.checks.size(); ++k) {
            const uint32_t position = plan.checks[k] & 0xFFFFu, id = plan.checks[k] >> 16;
            expect(position < n && 4 * (size_t)id < plan.bitmaps.size() && !listed[position], "entry");
            if (!(position < n && 4 * (size_t)id < plan.bitmaps.size())) continue;
            listed[position] = true;
            expect(std::memcmp(&plan.bitmaps[4 * id], &sets[4 * position], 32) == 0, "entry names the position's set");
            uint64_t sum = 0;
            for (unsigned b = 0; b < 256; ++b)
                if (set_has(&sets[4 * position], b)) sum += (uint64_t)cost[b];
            expect(k == 0 || before_cost < sum || (before_cost == sum && before_position < position), "rarest first, ties by position");
            before_cost = sum;
            before_position = position;
        }
        for (uint32_t p : inexact_positions) expect(listed[p], "every inexact position is listed");
    }
    // the limits at n = 4096: digits are inexact; {b, b + 3} with b & 3 == 0 is inexact too (its cover accepts four values)
    Set digits = Set{{0, 0, 0, 0}}, letter = Set{{0, 0, 0, 0}};
    set_add_range(digits, '0', '9');
    set_add(letter, 'q');
    for (size_t inexact : {kMaxInexact, kMaxInexact + 1}) {
        std::vector<uint64_t> sets(4 * kMaxLen);
        for (size_t i = 0; i < kMaxLen; ++i) std::memcpy(&sets[4 * i], (i % 3 == 1 && i / 3 < inexact ? digits : letter).w, 32);
        Plan plan;
        size_t where = 0;
        expect(make_class_plan(sets.data(), kMaxLen, cost, &plan, &where) == (inexact == kMaxInexact ? kPlanOk : kPlanTooManyInexact), "inexact limit");
    }
    for (size_t distinct : {kMaxDistinct, kMaxDistinct + 1}) {
        std::vector<uint64_t> sets(4 * kMaxLen);
        for (size_t i = 0; i < kMaxLen; ++i) {
            Set s = Set{{0, 0, 0, 0}};
            const unsigned id = (unsigned)(i % distinct), b = id < 64 ? 4 * id : 1;     // (the 65th: {1, 2})
            set_add(s, b);
            if (i < 1000) set_add(s, id < 64 ? b + 3 : 2);
            std::memcpy(&sets[4 * i], s.w, 32);
        }
        Plan plan;
        size_t where = 0;
        const PlanResult r = make_class_plan(sets.data(), kMaxLen, cost, &plan, &where);
        expect(r == (distinct == kMaxDistinct ? kPlanOk : kPlanTooManyDistinct), "distinct limit");
        if (r == kPlanOk) expect(plan.bitmaps.size() == 4 * kMaxDistinct && plan.inexact == 1000, "distinct count");
    }
    std::vector<uint64_t> empty(8, 0);
    empty[0] = 2;
    Plan plan;
    size_t where = 99;
    expect(make_class_plan(empty.data(), 2, cost, &plan, &where) == kPlanEmptySet && where == 1, "empty set");
}

int main()
{
    sweep_parser();
    sweep_cover();
    sweep_plan();
    std::printf("%ld checks, %ld failures\n", checks, failures);
    return failures > 100 ? 100 : (int)failures;
}
