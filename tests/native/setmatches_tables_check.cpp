// setmatches_tables_check.cpp - needle identity in the compiled set (sliceslice-rs_amd/csrc/needleset_tables.hpp: rank_of, the ranks
// of the entries and of the one- and two-byte needles, the histogram slots, set_each_at) on the host, against a brute-force memcmp
// loop.  A program of its own: tests/test_setmatches_cpu.py compiles it with ASan and UBSan and runs it.
//
//   small sets   every set of one or two needles of 1 .. 3 bytes and random sets of up to six needles of 1 .. 7 bytes (duplicates
//                and fold-equal needles among them) over alphabets of 2 - 3 bytes, with and without the fold, `how` 0 and WORD:
//                at every position of haystacks over the alphabet, set_each_at reports exactly the needles that occur there, each
//                once, in ascending rank - with the view alone in an allocation of exactly its size (ASan guards both ends), and
//                inside a larger buffer whose bytes around it are word bytes and needle copies that must not count.
//   large sets   300 needles that share one two-byte key, lengths up to 2,000, on haystacks that hold some of them.
//   slots        more than kSetHotSlots needles: the one- and two-byte ones hold the first slots, the longer ones follow in
//                ascending length, hot[slot[r]] == r, and a rank beyond the bins has none.
#include "../../sliceslice-rs_amd/csrc/needleset_tables.hpp"

#include <cstdio>
#include <cstdlib>
#include <memory>
#include <string>

using ss::SetTables;
typedef std::basic_string<uint8_t> Bytes;

static unsigned long long g_checks = 0, g_failures = 0;
static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint32_t rnd(uint32_t n)
{
    g_rng ^= g_rng << 13;
    g_rng ^= g_rng >> 7;
    g_rng ^= g_rng << 17;
    return (uint32_t)((g_rng >> 20) % n);
}

static uint8_t fold1(uint8_t b, bool fold) { return fold && b >= 'A' && b <= 'Z' ? (uint8_t)(b + 32) : b; }
static bool wordb(uint8_t b) { return (b >= '0' && b <= '9') || (b >= 'A' && b <= 'Z') || (b >= 'a' && b <= 'z') || b == '_'; }

static void fail(const char *what)
{
    if (++g_failures <= 20) std::printf("FAIL %s\n", what);
}

static bool build(const std::vector<Bytes> &needles, bool fold, SetTables *t)
{
    std::vector<const void *> p;
    std::vector<size_t> l;
    for (const Bytes &n : needles) {
        p.push_back(n.empty() ? nullptr : n.data());
        l.push_back(n.size());
    }
    return ss::set_build(p.data(), l.data(), (uint32_t)needles.size(), fold, t) == ss::kSetBuilt;
}

// the sorted, deduplicated order, restated: std::basic_string<uint8_t> compares bytes as unsigned and a prefix first
static std::vector<Bytes> distinct_of(const std::vector<Bytes> &needles, bool fold)
{
    std::vector<Bytes> f;
    for (Bytes n : needles) {
        for (auto &b : n) b = fold1(b, fold);
        f.push_back(n);
    }
    std::sort(f.begin(), f.end());
    f.erase(std::unique(f.begin(), f.end()), f.end());
    return f;
}

// rank_of, the ranks of the entries, of the one-byte and of the two-byte needles, and the slots
static void check_ranks(const SetTables &t, const std::vector<Bytes> &needles, bool fold)
{
    const std::vector<Bytes> f = distinct_of(needles, fold);
    ++g_checks;
    if (t.rank_of.size() != needles.size() || t.slot.size() != f.size() || t.erank.size() != t.entry.size() || t.rank1.size() != 256 ||
        t.key2.size() != t.two_byte || t.rank2.size() != t.two_byte)
        return fail("sizes of the rank tables");
    for (size_t k = 0; k < needles.size(); ++k) {
        Bytes n = needles[k];
        for (auto &b : n) b = fold1(b, fold);
        const size_t want = (size_t)(std::lower_bound(f.begin(), f.end(), n) - f.begin());
        ++g_checks;
        if (t.rank_of[k] != want) fail("rank_of");
    }
    for (size_t e = 0; e < t.entry.size(); ++e) {
        const ss::SetEntry &en = t.entry[e];
        ++g_checks;
        if (t.erank[e] >= f.size() || f[t.erank[e]] != Bytes(t.blob.data() + en.off, en.len)) fail("rank of an entry");
    }
    const ss::SetRanks r = t.ranks();
    size_t ones = 0;
    for (uint32_t b = 0; b < 256; ++b) {
        const bool has = ss::set_b1_bit(t.b1.data(), b) != 0;
        ++g_checks;
        if (has != (t.rank1[b] != ss::kSetNoSlot) || (has && f[t.rank1[b]] != Bytes(1, (uint8_t)b))) fail("rank of a one-byte needle");
        ones += has;
    }
    for (size_t i = 0; i < t.key2.size(); ++i) {
        const uint8_t two[2] = {(uint8_t)(t.key2[i] & 0xFF), (uint8_t)(t.key2[i] >> 8)};
        ++g_checks;
        if ((i != 0 && t.key2[i - 1] >= t.key2[i]) || f[t.rank2[i]] != Bytes(two, 2) || ss::set_rank2(r, t.key2[i]) != t.rank2[i])
            fail("rank of a two-byte needle");
    }
    // slots: a bijection between the hot ranks and [0, nhot); short needles first, then ascending length; full or everything
    const size_t real = f.size() - (t.every ? 1 : 0);
    ++g_checks;
    if (t.hot.size() != std::min<size_t>(real, ss::kSetHotSlots)) fail("number of hot slots");
    size_t slotted = 0;
    for (size_t rk = 0; rk < f.size(); ++rk) {
        const uint32_t s = t.slot[rk];
        if (s == ss::kSetNoSlot) continue;
        ++slotted;
        ++g_checks;
        if (s >= t.hot.size() || t.hot[s] != rk || f[rk].empty()) fail("slot and hot disagree");
    }
    ++g_checks;
    if (slotted != t.hot.size()) fail("slots are no bijection");
    for (size_t s = 1; s < t.hot.size(); ++s) {
        const size_t a = f[t.hot[s - 1]].size(), b = f[t.hot[s]].size();
        ++g_checks;
        if (a > b && !(a <= 2 && b <= 2)) fail("hot slots do not ascend in length");
    }
    if (t.hot.size() == ss::kSetHotSlots) {                     // no needle without a slot is shorter than one with a slot
        const size_t longest = f[t.hot.back()].size();
        for (size_t rk = 0; rk < f.size(); ++rk) {
            ++g_checks;
            if (t.slot[rk] == ss::kSetNoSlot && !f[rk].empty() && f[rk].size() < longest) fail("a shorter needle was left without a slot");
        }
    }
    (void)ones;
}

// every position of `hay` as a view of its own allocation, and as a view inside `around` + hay + `around`
static void check_view(const SetTables &t, const std::vector<Bytes> &needles, bool fold, const Bytes &hay, const Bytes &around)
{
    const ss::SetView v = t.view();
    const ss::SetRanks r = t.ranks();
    const std::vector<Bytes> f = distinct_of(needles, fold);
    std::unique_ptr<uint8_t[]> exact(new uint8_t[hay.size() ? hay.size() : 1]);
    if (!hay.empty()) std::memcpy(exact.get(), hay.data(), hay.size());
    const Bytes wide = around + hay + around;
    Bytes hf = hay;
    for (auto &b : hf) b = fold1(b, fold);
    const size_t len = hay.size();
    std::vector<uint32_t> want, got;
    for (unsigned how = 0; how <= 1; ++how) {
        for (size_t g = 0; g < len; ++g) {
            want.clear();
            for (size_t rk = 0; rk < f.size(); ++rk) {
                const Bytes &n = f[rk];
                if (n.empty() || n.size() > len - g || std::memcmp(hf.data() + g, n.data(), n.size()) != 0) continue;
                const size_t e = g + n.size();
                if (how != 0 && ((g > 0 && wordb(hay[g - 1])) || (e < len && wordb(hay[e])))) continue;
                want.push_back((uint32_t)rk);
            }
            for (int where = 0; where < 2; ++where) {
                got.clear();
                ss::set_each_at(v, r, where ? wide.data() + around.size() : exact.get(), len, g, how, [&](uint32_t rank) { got.push_back(rank); });
                ++g_checks;
                if (got != want) {                              // (`want` ascends and holds no rank twice)
                    if (++g_failures <= 20) {
                        std::printf("FAIL set_each_at %s: g=%zu how=%u fold=%d hay=", where ? "inside a buffer" : "exact", g, how, (int)fold);
                        for (uint8_t b : hay) std::printf("%02x", b);
                        std::printf(" got %zu want %zu\n", got.size(), want.size());
                    }
                }
            }
        }
    }
}

static void all_strings(const Bytes &alphabet, size_t least, size_t most, std::vector<Bytes> *out)
{
    std::vector<Bytes> all(1, Bytes());
    for (size_t b = 0, e = 1, n = 1; n <= most; ++n) {
        for (size_t k = b; k < e; ++k)
            for (uint8_t c : alphabet) all.push_back(all[k] + c);
        b = e;
        e = all.size();
    }
    for (const Bytes &s : all)
        if (s.size() >= least) out->push_back(s);
}

static Bytes random_string(const Bytes &alphabet, size_t n)
{
    Bytes s;
    for (size_t i = 0; i < n; ++i) s += alphabet[rnd((uint32_t)alphabet.size())];
    return s;
}

static void small_sets(const Bytes &alphabet, bool fold)
{
    std::vector<Bytes> short_needles, hays;
    all_strings(alphabet, 1, 3, &short_needles);
    all_strings(alphabet, 0, alphabet.size() == 2 ? 7 : 5, &hays);
    const Bytes around = alphabet + alphabet + Bytes((const uint8_t *)"x_", 2) + alphabet;
    SetTables t;
    for (size_t a = 0; a < short_needles.size(); ++a) {
        for (size_t b = a; b < short_needles.size(); b += (alphabet.size() == 2 ? 2 : 7)) {
            const std::vector<Bytes> needles = {short_needles[a], short_needles[b]};
            if (!build(needles, fold, &t)) { fail("build"); continue; }
            check_ranks(t, needles, fold);
            for (size_t h = (a * 7 + b) % 11; h < hays.size(); h += 11) check_view(t, needles, fold, hays[h], around);
        }
    }
    for (int round = 0; round < 300; ++round) {
        std::vector<Bytes> needles;
        for (uint32_t k = 1 + rnd(6); k > 0; --k) needles.push_back(random_string(alphabet, 1 + rnd(7)));
        if (rnd(3) == 0) needles.push_back(needles[rnd((uint32_t)needles.size())]);             // a duplicate
        if (rnd(3) == 0) needles.push_back(needles[0].substr(0, 1 + rnd((uint32_t)needles[0].size())));       // a prefix
        if (!build(needles, fold, &t)) { fail("build"); continue; }
        check_ranks(t, needles, fold);
        for (int h = 0; h < 12; ++h) {
            Bytes hay = random_string(alphabet, rnd(25));
            if (!hay.empty() && rnd(2)) {                       // a needle planted at a random place, also across the end
                const Bytes &n = needles[rnd((uint32_t)needles.size())];
                const size_t at = rnd((uint32_t)hay.size());
                hay = hay.substr(0, at) + n + hay.substr(at);
                if (rnd(4) == 0) hay.resize(hay.size() - rnd((uint32_t)hay.size()));
            }
            check_view(t, needles, fold, hay, around);
        }
    }
}

static void large_sets(bool fold)
{
    const Bytes alphabet((const uint8_t *)"abcQ", 4);
    for (int round = 0; round < 6; ++round) {
        std::vector<Bytes> needles;
        for (int k = 0; k < 300; ++k) {
            const size_t n = k < 8 ? 1994 + (size_t)k : 3 + rnd(k % 3 ? 8 : 1990);
            needles.push_back(Bytes((const uint8_t *)"qa", 2) + random_string(alphabet, n - 2));
        }
        // a chain of prefixes of one long needle: all of them occur where it does
        for (size_t n = 3; n < 40; n += 5) needles.push_back(needles[0].substr(0, n));
        needles.push_back(Bytes((const uint8_t *)"q", 1));
        needles.push_back(Bytes((const uint8_t *)"qa", 2));
        needles.push_back(Bytes((const uint8_t *)"ab", 2));
        SetTables t;
        if (!build(needles, fold, &t)) { fail("build"); continue; }
        check_ranks(t, needles, fold);
        if (t.largest_bucket < 200) fail("largest bucket");
        for (int h = 0; h < 6; ++h) {
            Bytes hay = random_string(alphabet, 40);
            const Bytes &n = needles[h == 0 ? 0 : rnd(300)];
            hay += h % 3 == 2 ? n.substr(0, n.size() - 1) : n;                   // (one byte short: no match of this needle)
            if (h % 2) hay += random_string(alphabet, 30);
            if (h == 5) hay[hay.size() / 2] = ' ';
            check_view(t, needles, fold, hay, Bytes((const uint8_t *)"qa q", 4));
        }
    }
}

// more needles than bins: 17^3 three-byte needles, then the same with one- and two-byte needles and longer ones added
static void slots()
{
    const Bytes letters((const uint8_t *)"abcdefghijklmnopq", 17);
    std::vector<Bytes> needles;
    all_strings(letters, 3, 3, &needles);
    SetTables t;
    if (!build(needles, false, &t)) return fail("build");
    check_ranks(t, needles, false);
    ++g_checks;
    if (t.distinct != 4913 || t.hot.size() != ss::kSetHotSlots) fail("4,913 needles fill the bins");
    for (int k = 0; k < 200; ++k) needles.push_back(random_string(letters, 1 + rnd(2)));
    for (int k = 0; k < 50; ++k) needles.push_back(random_string(letters, 4 + rnd(5)));
    if (!build(needles, false, &t)) return fail("build");
    check_ranks(t, needles, false);
    const std::vector<Bytes> f = distinct_of(needles, false);
    for (size_t rk = 0; rk < f.size(); ++rk) {
        ++g_checks;
        if (f[rk].size() <= 2 && t.slot[rk] >= t.one_byte + t.two_byte) fail("a short needle is not among the first slots");
        if (f[rk].size() > 3 && t.slot[rk] != ss::kSetNoSlot) fail("a long needle holds a slot while three-byte needles have none");
    }
    const Bytes hay = random_string(letters, 400);
    check_view(t, needles, false, hay, Bytes((const uint8_t *)"abc", 3));
}

int main()
{
    for (int fold = 0; fold <= 1; ++fold) {
        small_sets(Bytes((const uint8_t *)"ab", 2), fold != 0);
        small_sets(Bytes((const uint8_t *)"aA", 2), fold != 0);
        small_sets(Bytes((const uint8_t *)"aAb", 3), fold != 0);
        small_sets(Bytes((const uint8_t *)"a_ ", 3), fold != 0);
        small_sets(Bytes((const uint8_t *)"Z .", 3), fold != 0);
        large_sets(fold != 0);
    }
    slots();
    // what the issue's example says in so many words
    SetTables t;
    const std::vector<Bytes> five = {Bytes((const uint8_t *)"ab", 2), Bytes((const uint8_t *)"abb", 3), Bytes((const uint8_t *)"abba", 4),
                                     Bytes((const uint8_t *)"ab", 2), Bytes((const uint8_t *)"AB", 2)};
    ++g_checks;
    if (!build(five, false, &t) || t.rank_of != std::vector<uint32_t>({1, 2, 3, 1, 0})) fail("ranks of {ab, abb, abba, ab, AB}");
    ++g_checks;
    if (!build(five, true, &t) || t.rank_of != std::vector<uint32_t>({0, 1, 2, 0, 0})) fail("ranks of {ab, abb, abba, ab, AB} folded");
    std::printf("setmatches_tables_check: %llu checks, %llu failures\n", g_checks, g_failures);
    return g_failures == 0 ? 0 : 1;
}
