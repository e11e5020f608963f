// leftmost_host_check.cpp - a sweep of sliceslice-rs_amd/csrc/leftmost_host.hpp against brute force, compiled for the host alone
// (tests/test_leftmost_cpu.py builds it with -fsanitize=address,undefined and runs it as a child):
//   * select_leftmost_host against a walk over a byte-wise occupancy map, for every text over {a, b} up to length 10 with the needle
//     sets {a, ab, abb}, {b, ba}, {ab, b, bab, a} as the lists of (offset, length) entries, at every capacity, with sentinels
//     behind the capacity;
//   * rank_replacements with equal and conflicting duplicates, and with a rank beyond the table;
//   * replaced_set_length at the edges of 64 bits;
//   * replaced_starts_host and the length against a byte-wise loop that writes the substituted text.
// Prints "<checks> checks, <failures> failures" and exits with the number of failures (capped).
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../sliceslice-rs_amd/csrc/leftmost_host.hpp"

static unsigned long long g_checks = 0, g_failures = 0;

static void check(bool ok, const char *what, unsigned long long a, unsigned long long b)
{
    ++g_checks;
    if (ok) return;
    if (++g_failures <= 20) std::printf("FAIL %s (%llu, %llu)\n", what, a, b);
}

int main()
{
    const std::vector<std::vector<std::string>> sets = {{"a", "ab", "abb"}, {"b", "ba"}, {"a", "ab", "b", "bab"}};      // (each sorted: ranks ascend)
    const std::vector<std::vector<std::string>> texts_for = {{"", "xy", "0123456789"}, {"<>", ""}, {"q", "", "longer than any", "zz"}};
    const uint64_t sentinel = 0xA5A5A5A5A5A5A5A5ull;
    for (size_t si = 0; si < sets.size(); ++si) {
        const std::vector<std::string> &needles = sets[si];
        for (size_t n = 0; n <= 10; ++n)
            for (unsigned bits = 0; bits < (1u << n); ++bits) {
                std::string text(n, 'a');
                for (size_t i = 0; i < n; ++i)
                    if (bits >> i & 1) text[i] = 'b';
                // the pairs as ss_find_all_set_device lists them: by offset, then by rank
                std::vector<uint64_t> offsets, lengths, ranks;
                for (size_t p = 0; p < n; ++p)
                    for (size_t r = 0; r < needles.size(); ++r)
                        if (text.compare(p, needles[r].size(), needles[r]) == 0 && p + needles[r].size() <= n) {
                            offsets.push_back(p);
                            lengths.push_back(needles[r].size());
                            ranks.push_back(r);
                        }
                // brute force: at every free byte the longest needle that stands there
                std::vector<uint64_t> want, want_rank;
                for (size_t p = 0; p < n;) {
                    size_t best = needles.size();
                    for (size_t r = 0; r < needles.size(); ++r)
                        if (p + needles[r].size() <= n && text.compare(p, needles[r].size(), needles[r]) == 0 &&
                            (best == needles.size() || needles[r].size() > needles[best].size()))
                            best = r;
                    if (best == needles.size()) {
                        ++p;
                    } else {
                        want.push_back(p);
                        want_rank.push_back(best);
                        p += needles[best].size();
                    }
                }
                std::vector<uint64_t> which(want.size() + 2);
                for (uint64_t capacity = 0; capacity <= want.size() + 1; ++capacity) {
                    std::vector<uint64_t> got(want.size() + 2, sentinel);
                    std::fill(which.begin(), which.end(), sentinel);
                    const uint64_t total = ssh::select_leftmost_host(offsets.data(), lengths.data(), offsets.size(), got.data(), which.data(), capacity);
                    check(total == want.size(), "the selection's size", n, bits);
                    for (uint64_t k = 0; k < got.size(); ++k) {
                        const bool inside = k < capacity && k < want.size();
                        check(got[k] == (inside ? want[k] : sentinel), "a selected offset", n, bits);
                        check(inside ? (which[k] < offsets.size() && ranks[which[k]] == want_rank[k] && offsets[which[k]] == want[k]) : which[k] == sentinel,
                              "a selected index", n, bits);
                    }
                }
                check(ssh::select_leftmost_host(offsets.data(), lengths.data(), offsets.size(), nullptr, nullptr, 5) == want.size(), "count only", n, bits);
                // the substituted text, byte by byte, against the starts and the length
                const std::vector<std::string> &reps = texts_for[si];
                std::string out;
                std::vector<uint64_t> want_starts, nl, rl;
                size_t at = 0;
                for (size_t k = 0; k < want.size(); ++k) {
                    for (; at < want[k]; ++at) out.push_back(text[at]);
                    want_starts.push_back(out.size());
                    out += reps[want_rank[k]];
                    at += needles[want_rank[k]].size();
                    nl.push_back(needles[want_rank[k]].size());
                    rl.push_back(reps[want_rank[k]].size());
                }
                for (; at < n; ++at) out.push_back(text[at]);
                std::vector<uint64_t> starts(want.size() + 1, sentinel);
                const uint64_t delta = ssh::replaced_starts_host(want.data(), nl.data(), rl.data(), want.size(), starts.data());
                check(starts == [&] { std::vector<uint64_t> w = want_starts; w.push_back(sentinel); return w; }(), "the starts", n, bits);
                uint64_t out_len = 0;
                check(ssh::replaced_set_length(n, want.size(), 15, delta, &out_len) && out_len == out.size(), "the length", n, bits);
            }
    }
    // ---- the replacement of every rank ----
    {
        const uint32_t rank_of[5] = {2, 0, 2, 1, 0};
        const char *a = "same", *b = "same", *c = "other", *e = "";
        std::vector<uint32_t> owner;
        const void *equal[5] = {a, c, b, e, c};
        const size_t equal_lens[5] = {4, 5, 4, 0, 5};
        check(ssh::rank_replacements(rank_of, 5, equal, equal_lens, 3, &owner) == -1, "equal duplicates", 0, 0);
        check(owner.size() == 3 && owner[0] == 1 && owner[1] == 3 && owner[2] == 0, "the first needle of a rank owns it", 0, 0);
        const void *differ[5] = {a, c, c, e, c};
        const size_t differ_lens[5] = {4, 5, 5, 0, 5};
        check(ssh::rank_replacements(rank_of, 5, differ, differ_lens, 3, &owner) == 2, "a conflicting duplicate", 0, 0);
        const size_t shorter_lens[5] = {4, 5, 4, 0, 4};
        check(ssh::rank_replacements(rank_of, 5, equal, shorter_lens, 3, &owner) == 4, "a duplicate of another length", 0, 0);
        const void *nulls[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
        const size_t zeros[5] = {0, 0, 0, 0, 0};
        check(ssh::rank_replacements(rank_of, 5, nulls, zeros, 3, &owner) == -1, "empty replacements may be NULL", 0, 0);
        check(ssh::rank_replacements(rank_of, 5, equal, equal_lens, 2, &owner) == 0, "a rank beyond the table", 0, 0);
        check(ssh::rank_replacements(rank_of, 0, equal, equal_lens, 0, &owner) == -1 && owner.empty(), "no needle", 0, 0);
    }
    // ---- the length at the edges of 64 bits ----
    {
        uint64_t out = 7;
        check(ssh::replaced_set_length(100, 0, UINT64_MAX, 0, &out) && out == 100, "no selection", 0, 0);
        check(ssh::replaced_set_length(UINT64_MAX, 0, 5, 0, &out) && out == UINT64_MAX, "no selection of the largest view", 0, 0);
        check(ssh::replaced_set_length(10, 3, 0, (uint64_t)0 - 6, &out) && out == 4, "deletions", 0, 0);
        check(ssh::replaced_set_length(10, 2, (UINT64_MAX - 10) / 2, 2 * ((UINT64_MAX - 10) / 2) - 4, &out) && out == 10 + 2 * ((UINT64_MAX - 10) / 2) - 4,
              "the largest that fits", 0, 0);
        out = 7;
        check(!ssh::replaced_set_length(10, 2, (UINT64_MAX - 10) / 2 + 1, 0, &out) && out == 7, "one more does not", 0, 0);
        check(!ssh::replaced_set_length(UINT64_MAX, 1, 1, 0, &out) && out == 7, "no room behind the largest view", 0, 0);
        check(ssh::replaced_set_length(UINT64_MAX - 1, 1, 1, 0, &out) && out == UINT64_MAX - 1, "one byte of room", 0, 0);
    }
    std::printf("%llu checks, %llu failures\n", g_checks, g_failures);
    return g_failures > 100 ? 100 : (int)g_failures;
}
