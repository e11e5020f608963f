// context_ranges_check.cpp - the range arithmetic of the context calls (sliceslice-rs_amd/csrc/context_ranges.hpp) on the host,
// against a brute-force union.  A stand-alone program: tests/test_context_cpu.py compiles it for the host with
// -fsanitize=address,undefined and runs it as a child process.
//
//   every N <= 6, every subset S of 1 .. N, b and a in {0, 1, 2, 5, 2^64 - 1}: the owned ranges are disjoint, ascending, and
//   their union with kinds is the brute-force one; the exclusive prefix of their sizes is every entry's first slot
//   the same with an entry 0 in front and entries N + 1, N + 2 behind: they own nothing and change nothing
//   saturation at the ends of uint64_t, and neighbours out of order (a breach of the caller's contract): every range stays in [1, N]
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../sliceslice-rs_amd/csrc/context_ranges.hpp"

static long g_checks = 0, g_failures = 0;

#define EXPECT(cond, ...)                                   \
    do {                                                    \
        ++g_checks;                                         \
        if (!(cond)) {                                      \
            if (++g_failures <= 20) {                       \
                std::printf("FAIL %s: ", #cond);            \
                std::printf(__VA_ARGS__);                   \
                std::printf("\n");                          \
            }                                               \
        }                                                   \
    } while (0)

static void sweep(const std::vector<uint64_t> &entries, uint64_t N, uint64_t b, uint64_t a)
{
    // brute force: line k is printed when some valid entry s has s - b <= k <= s + a (in unbounded integers)
    std::vector<int> want_kind(N + 2, -1);
    for (uint64_t k = 1; k <= N; ++k) {
        for (uint64_t s : entries) {
            if (s < 1 || s > N) continue;
            const bool near = k <= s ? (s - k <= b) : (k - s <= a);
            if (near && want_kind[k] < 0) want_kind[k] = 0;
            if (s == k) want_kind[k] = 1;
        }
    }
    std::vector<uint64_t> got_line;
    std::vector<int> got_kind;
    uint64_t slot = 0;
    for (size_t i = 0; i < entries.size(); ++i) {
        const uint64_t prev = i > 0 ? entries[i - 1] : 0, next = i + 1 < entries.size() ? entries[i + 1] : 0;
        const ss::CtxRange r = ss::ctx_range(prev, entries[i], next, N, b, a);
        const uint64_t size = ss::ctx_size(r);
        if (entries[i] < 1 || entries[i] > N) {
            EXPECT(size == 0, "entry %llu of N %llu owns %llu lines", (unsigned long long)entries[i], (unsigned long long)N, (unsigned long long)size);
            continue;
        }
        EXPECT(size >= 1 && r.lo >= 1 && r.hi <= N && r.lo <= entries[i] && entries[i] <= r.hi, "N %llu s %llu: [%llu, %llu]",
               (unsigned long long)N, (unsigned long long)entries[i], (unsigned long long)r.lo, (unsigned long long)r.hi);
        EXPECT(got_line.empty() || r.lo > got_line.back(), "N %llu s %llu: lo %llu not behind %llu", (unsigned long long)N,
               (unsigned long long)entries[i], (unsigned long long)r.lo, (unsigned long long)(got_line.empty() ? 0 : got_line.back()));
        EXPECT(slot == got_line.size(), "prefix");
        for (uint64_t k = r.lo; k <= r.hi && k >= r.lo; ++k) {
            got_line.push_back(k);
            got_kind.push_back(k == entries[i] ? 1 : 0);
        }
        slot += size;
    }
    std::vector<uint64_t> want_line;
    std::vector<int> kinds;
    for (uint64_t k = 1; k <= N; ++k)
        if (want_kind[k] >= 0) {
            want_line.push_back(k);
            kinds.push_back(want_kind[k]);
        }
    EXPECT(got_line == want_line && got_kind == kinds, "N %llu b %llu a %llu entries %zu: %zu lines, want %zu", (unsigned long long)N,
           (unsigned long long)b, (unsigned long long)a, entries.size(), got_line.size(), want_line.size());
}

int main()
{
    const uint64_t amounts[] = {0, 1, 2, 5, ~0ull};
    for (uint64_t N = 0; N <= 6; ++N)
        for (uint64_t mask = 0; mask < (1ull << N); ++mask)
            for (uint64_t b : amounts)
                for (uint64_t a : amounts) {
                    std::vector<uint64_t> s;
                    for (uint64_t k = 1; k <= N; ++k)
                        if (mask >> (k - 1) & 1) s.push_back(k);
                    sweep(s, N, b, a);
                    std::vector<uint64_t> wide;                 // 0 in front, N + 1 and N + 2 behind: still strictly ascending
                    wide.push_back(0);
                    wide.insert(wide.end(), s.begin(), s.end());
                    wide.push_back(N + 1);
                    wide.push_back(N + 2);
                    sweep(wide, N, b, a);
                }
    // saturation at the ends of uint64_t
    const uint64_t top = ~0ull;
    EXPECT(ss::ctx_sat_add(top, 1) == top && ss::ctx_sat_add(top - 1, 1) == top && ss::ctx_sat_add(3, 4) == 7, "sat_add");
    EXPECT(ss::ctx_sat_sub(0, 1) == 0 && ss::ctx_sat_sub(3, top) == 0 && ss::ctx_sat_sub(9, 4) == 5, "sat_sub");
    {
        const ss::CtxRange r = ss::ctx_range(top - 2, top - 1, top, top, top, top);
        EXPECT(r.lo == top - 1 && r.hi == top - 1, "neighbours at the top: [%llu, %llu]", (unsigned long long)r.lo, (unsigned long long)r.hi);
        const ss::CtxRange all = ss::ctx_range(0, top, 0, top, top, top);
        EXPECT(all.lo == 1 && all.hi == top && ss::ctx_size(all) == top, "one entry at the top");
    }
    // neighbours out of order are ignored: the range stays inside [1, N] and holds the entry
    for (uint64_t N = 1; N <= 5; ++N)
        for (uint64_t s = 1; s <= N; ++s)
            for (uint64_t prev = 0; prev <= N + 2; ++prev)
                for (uint64_t next = 0; next <= N + 2; ++next)
                    for (uint64_t b : amounts)
                        for (uint64_t a : amounts) {
                            const ss::CtxRange r = ss::ctx_range(prev, s, next, N, b, a);
                            EXPECT(r.lo >= 1 && r.hi <= N && r.lo <= s && s <= r.hi, "breach N %llu s %llu prev %llu next %llu",
                                   (unsigned long long)N, (unsigned long long)s, (unsigned long long)prev, (unsigned long long)next);
                        }
    std::printf("%ld checks, %ld failures\n", g_checks, g_failures);
    return g_failures ? 1 : 0;
}
