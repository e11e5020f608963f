// disjoint_host_check.cpp - a sweep of sliceslice-rs_amd/csrc/disjoint_host.hpp against brute force, compiled for the host alone
// (tests/test_disjoint_cpu.py builds it with -fsanitize=address,undefined and runs it as a child):
//   * longest_proper_border against the quadratic definition, for every needle over {a, b} up to length 10, and its meaning: two
//     occurrences of the needle overlap somewhere in some text if and only if the border is above 0;
//   * select_disjoint_host against the obvious loop, for every subset of a 14-byte window as the offsets and n = 1 .. 15, at every
//     capacity that cuts the selection, with sentinels behind the capacity;
//   * replaced_length at the edges of 64 bits.
// Prints "<checks> checks, <failures> failures" and exits with the number of failures (capped).
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../sliceslice-rs_amd/csrc/disjoint_host.hpp"

static unsigned long long g_checks = 0, g_failures = 0;

static void check(bool ok, const char *what, unsigned long long a, unsigned long long b)
{
    ++g_checks;
    if (ok) return;
    if (++g_failures <= 20) std::printf("FAIL %s (%llu, %llu)\n", what, a, b);
}

static size_t border_quadratic(const std::string &s)
{
    for (size_t k = s.size() - 1; k > 0; --k)
        if (std::memcmp(s.data(), s.data() + s.size() - k, k) == 0) return k;
    return 0;
}

int main()
{
    // ---- the border ----
    for (size_t n = 0; n <= 10; ++n)
        for (unsigned bits = 0; bits < (1u << n); ++bits) {
            std::string needle(n, 'a');
            for (size_t i = 0; i < n; ++i)
                if (bits >> i & 1) needle[i] = 'b';
            const size_t got = ssh::longest_proper_border(reinterpret_cast<const uint8_t *>(needle.data()), n);
            check(got == (n ? border_quadratic(needle) : 0), "border", n, bits);
            if (n == 0) continue;
            // the text needle + needle[border:] holds a second occurrence at n - border < n exactly when the border is above 0
            const std::string text = needle + needle.substr(got);
            size_t found = 0;
            for (size_t p = 1; p < n && p + n <= text.size(); ++p)
                if (text.compare(p, n, needle) == 0) ++found;
            check((found != 0) == (got != 0), "border means overlap", n, bits);
        }
    // ---- the greedy walk ----
    const unsigned window = 14;
    std::vector<uint64_t> offsets, want, got(window + 2);
    for (unsigned subset = 0; subset < (1u << window); ++subset) {
        offsets.clear();
        for (unsigned i = 0; i < window; ++i)
            if (subset >> i & 1) offsets.push_back(1000 + i);
        for (uint64_t n = 1; n <= window + 1; ++n) {
            want.clear();
            for (size_t j = 0; j < offsets.size(); ++j)                     // the obvious loop
                if (want.empty() || offsets[j] - want.back() >= n) want.push_back(offsets[j]);
            const uint64_t total = ssh::select_disjoint_host(offsets.data(), offsets.size(), n, nullptr, 0);
            check(total == want.size(), "count", subset, n);
            const uint64_t caps[4] = {0, 1, want.size() ? want.size() - 1 : 0, want.size()};
            for (uint64_t cap : caps) {
                std::fill(got.begin(), got.end(), ~0ull);
                const uint64_t again = ssh::select_disjoint_host(offsets.data(), offsets.size(), n, got.data(), cap);
                bool ok = again == want.size();
                for (uint64_t k = 0; k < cap && k < want.size(); ++k) ok = ok && got[k] == want[k];
                for (uint64_t k = cap < want.size() ? cap : want.size(); k < got.size(); ++k) ok = ok && got[k] == ~0ull;
                check(ok, "offsets at a capacity", subset, n * 100 + cap);
            }
        }
    }
    // offsets at the top of 64 bits: p + n does not wrap
    {
        const uint64_t top[3] = {~0ull - 5, ~0ull - 3, ~0ull};
        uint64_t out[3] = {0, 0, 0};
        check(ssh::select_disjoint_host(top, 3, 4, out, 3) == 2 && out[0] == top[0] && out[1] == top[2], "near 2^64", 0, 0);
        check(ssh::select_disjoint_host(top, 3, ~0ull, out, 3) == 1, "n = 2^64 - 1", 0, 0);
        check(ssh::select_disjoint_host(top, 0, 1, out, 3) == 0, "empty list", 0, 0);
    }
    // ---- the output length ----
    {
        uint64_t len = 0;
        check(ssh::replaced_length(10, 3, 2, 0, &len) && len == 4, "shrink", len, 0);
        check(ssh::replaced_length(10, 3, 2, 5, &len) && len == 19, "grow", len, 0);
        check(ssh::replaced_length(10, 0, 2, ~0ull, &len) && len == 10, "no occurrence", len, 0);
        check(ssh::replaced_length(0, 0, 1, 1, &len) && len == 0, "empty view", len, 0);
        check(!ssh::replaced_length(10, 6, 2, 0, &len), "more than fit", 0, 0);
        check(!ssh::replaced_length(1ull << 40, 1ull << 39, 2, 1ull << 26, &len), "overflow", 0, 0);
        check(ssh::replaced_length(~0ull, 1, ~0ull, ~0ull, &len) && len == ~0ull, "the whole of 64 bits", len, 0);
        check(!ssh::replaced_length(~0ull, 1, ~0ull - 1, ~0ull, &len), "one too many", 0, 0);
    }
    std::printf("%llu checks, %llu failures\n", g_checks, g_failures);
    return g_failures > 100 ? 100 : (int)g_failures;
}
