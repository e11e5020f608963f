// output_host_check.cpp - a sweep of sliceslice-rs_amd/csrc/output_host.hpp, the arithmetic of the output rule, compiled for the
// host alone (tests/test_output_cpu.py builds it with -fsanitize=address,undefined and runs it as a child):
//   * out_digits, out_digit and out_write_decimal against snprintf at every power of ten, one below and one above it, at 0 and at
//     2^64 - 1, with sentinels around the written digits;
//   * out_clamp, out_separated, out_prefix and out_record_size against the rule written out as a loop, for every small case: views of
//     0 .. 6 bytes, begin and end 0 .. 8 and at the top of 64 bits, numbers 0 .. 5 and at the top of 64 bits, every flag combination,
//     terminators -1, 0 and 10, with and without a predecessor.
// Prints "<checks> checks, <failures> failures" and exits with the number of failures (capped).
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <string>

#include "../../sliceslice-rs_amd/csrc/output_host.hpp"

static unsigned long long g_checks = 0, g_failures = 0;

static void check(bool ok, const char *what, unsigned long long a, unsigned long long b)
{
    ++g_checks;
    if (ok) return;
    if (++g_failures <= 20) std::printf("FAIL %s (%llu, %llu)\n", what, a, b);
}

static void check_decimal(uint64_t v)
{
    char want[32];
    const int n = std::snprintf(want, sizeof want, "%" PRIu64, v);
    check(ss::out_digits(v) == n, "digits", v, (unsigned long long)n);
    uint8_t got[24];
    std::memset(got, 0xA5, sizeof got);
    const int wrote = ss::out_write_decimal(v, got + 2);
    bool ok = wrote == n && got[0] == 0xA5 && got[1] == 0xA5 && got[2 + n] == 0xA5 && got[23] == 0xA5;
    ok = ok && std::memcmp(got + 2, want, (size_t)n) == 0;
    check(ok, "decimal", v, (unsigned long long)wrote);
    for (int k = 0; k < n; ++k) check(ss::out_digit(v, n, k) == (uint8_t)want[k], "digit", v, (unsigned long long)k);
}

// the rule, written out: the bytes record (begin, end, number) contributes behind a record numbered `prev`
static uint64_t size_by_the_rule(unsigned flags, int terminator, bool first, uint64_t prev, uint64_t number, uint64_t begin, uint64_t end, uint64_t len)
{
    std::string out;
    // number > prev + 1 in unbounded arithmetic: prev + 1 is formed only where it does not wrap
    const bool separated = !first && prev != UINT64_MAX && number > prev + 1;
    if ((flags & 2u) && separated) {
        out += "--";
        if (terminator >= 0) out += (char)terminator;
    }
    if (flags & 1u) {
        char text[32];
        std::snprintf(text, sizeof text, "%" PRIu64, number);
        out += text;
        out += ':';
    }
    uint64_t count = 0;
    for (uint64_t p = begin; p < end && p < len; ++p) ++count;                  // (views here hold 6 bytes at the most)
    out.append((size_t)count, 'x');
    if (terminator >= 0) out += (char)terminator;
    return out.size();
}

int main()
{
    // ---- the decimal form ----
    check_decimal(0);
    check_decimal(UINT64_MAX);
    uint64_t p = 1;
    for (int k = 0; k < 20; ++k) {
        check(ss::out_pow10(k) == p, "pow10", (unsigned long long)k, p);
        check_decimal(p - 1);
        check_decimal(p);
        check_decimal(p + 1);
        if (k < 19) p *= 10u;
    }
    for (uint64_t v = 0; v < 200000; ++v) check_decimal(v);
    for (uint64_t v = UINT64_MAX - 1000; v != UINT64_MAX; ++v) check_decimal(v);
    // ---- the clamp, the separator and the size ----
    const uint64_t wide[] = {0, 1, 2, 3, 4, 5, 6, 7, 8, UINT64_MAX - 1, UINT64_MAX, 1ull << 63};
    const uint64_t numbers[] = {0, 1, 2, 3, 4, 5, 9, 10, 11, UINT64_MAX - 2, UINT64_MAX - 1, UINT64_MAX};
    const int terminators[] = {-1, 0, 10};
    for (uint64_t len = 0; len <= 6; ++len)
        for (uint64_t begin : wide)
            for (uint64_t end : wide) {
                uint64_t b = 77, e = 77;
                ss::out_clamp(begin, end, len, &b, &e);
                uint64_t count = 0;
                for (uint64_t q = 0; q < len; ++q) count += q >= begin && q < end;
                check(b <= e && e <= len && e - b == count && (count == 0 || b == begin), "clamp", begin, end);
                for (uint64_t prev : numbers)
                    for (uint64_t number : numbers) {
                        const bool separated = prev != UINT64_MAX && number > prev + 1;
                        check(ss::out_separated(prev, number) == separated, "separated", prev, number);
                        for (unsigned flags = 0; flags < 4; ++flags)
                            for (int terminator : terminators)
                                for (int first = 0; first < 2; ++first) {
                                    const uint64_t want = size_by_the_rule(flags, terminator, first != 0, prev, number, begin, end, len);
                                    const uint64_t got = ss::out_record_size(flags, terminator, first != 0, prev, number, begin, end, len);
                                    check(got == want, "size", flags * 100 + (unsigned)(terminator + 1), number);
                                    const ss::OutPrefix pre = ss::out_prefix(flags, terminator, first != 0, prev, number);
                                    check(pre.sep + pre.num + count + (terminator >= 0 ? 1u : 0u) == want && pre.sep <= 3 && pre.num <= 21, "prefix", flags, number);
                                }
                    }
            }
    std::printf("%llu checks, %llu failures\n", g_checks, g_failures);
    return g_failures > 100 ? 100 : (int)g_failures;
}
