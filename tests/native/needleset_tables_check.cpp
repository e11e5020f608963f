// needleset_tables_check.cpp - the needle set's tables and lookup (sliceslice-rs_amd/csrc/needleset_tables.hpp) on the host, against
// a brute-force memcmp loop.  A program of its own: tests/test_needleset_cpu.py compiles it with ASan and UBSan and runs it.
//
//   small sets   every set of one or two needles of 0 .. 3 bytes, and random sets of up to six needles of 0 .. 7 bytes, over
//                alphabets of 2 - 3 bytes, with and without the fold; the haystacks of 0 .. 7 bytes over the alphabet plus the
//                delimiter (every 23rd per set, from a start that moves with the set) or random ones of up to 24 bytes; the delimiter a byte of its own or a needle byte; every
//                `how`; the view alone in an allocation of exactly its size, and inside a larger buffer whose bytes around it are
//                word bytes, delimiters and needle copies that must not count.
//   letters      needles of 3 .. 12 bytes that hold a letter delimiter, in either case, at every index (the masked compare and the
//                byte loop), on their own bytes in both cases.
//   large sets   300 needles that share one two-byte key, lengths up to 2,000, on haystacks that hold some of them.
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

// the rule, restated: the folded haystack keeps its delimiters; a needle that holds the delimiter matches nothing
// (hf: the folded haystack; needles: folded, without the empty one and those that hold the delimiter)
static bool brute(const std::vector<Bytes> &needles, const Bytes &hf, const uint8_t *hay, size_t len, size_t g, int delim, unsigned how)
{
    for (const Bytes &n : needles) {
        if (n.size() > len - g) continue;
        if (std::memcmp(hf.data() + g, n.data(), n.size()) != 0) continue;
        bool ok = true;
        if (how != 0) {
            const size_t e = g + n.size();
            if (g > 0 && hay[g - 1] != delim && (how == ss::kSetLine || wordb(hay[g - 1]))) ok = false;
            if (e < len && hay[e] != delim && (how == ss::kSetLine || wordb(hay[e]))) ok = false;
        }
        if (ok) return true;
    }
    return false;
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

static void fail(const char *what, const std::vector<Bytes> &needles, const Bytes &hay, size_t g, int delim, unsigned how, bool fold)
{
    if (++g_failures > 20) return;
    std::printf("FAIL %s: g=%zu delim=%d how=%u fold=%d hay=", what, g, delim, how, (int)fold);
    for (uint8_t b : hay) std::printf("%02x", b);
    std::printf(" needles=");
    for (const Bytes &n : needles) {
        for (uint8_t b : n) std::printf("%02x", b);
        std::printf(",");
    }
    std::printf("\n");
}

// every position of `hay` as a view of its own allocation, and as a view inside `around` + hay + `around`
static void check_view(const SetTables &t, const std::vector<Bytes> &needles, bool fold, const Bytes &hay, int delim, const Bytes &around)
{
    const ss::SetView v = t.view();
    std::unique_ptr<uint8_t[]> exact(new uint8_t[hay.size() ? hay.size() : 1]);
    if (!hay.empty()) std::memcpy(exact.get(), hay.data(), hay.size());
    const Bytes wide = around + hay + around;
    Bytes hf = hay;
    for (auto &b : hf) b = b == delim ? b : fold1(b, fold);
    std::vector<Bytes> folded;
    for (Bytes n : needles) {
        for (auto &b : n) b = fold1(b, fold);
        if (!n.empty() && n.find((uint8_t)delim) == Bytes::npos) folded.push_back(n);
    }
    for (unsigned how = 0; how <= 2; ++how) {
        for (size_t g = 0; g < hay.size(); ++g) {
            const bool want = brute(folded, hf, hay.data(), hay.size(), g, delim, how);
            ++g_checks;
            if (ss::set_match_at(v, exact.get(), hay.size(), g, (uint32_t)delim, how) != want) fail("exact", needles, hay, g, delim, how, fold);
            if (ss::set_match_at(v, wide.data() + around.size(), hay.size(), g, (uint32_t)delim, how) != want)
                fail("inside a buffer", needles, hay, g, delim, how, fold);
        }
    }
}

static void check_tables(const SetTables &t, const std::vector<Bytes> &needles, bool fold)
{
    // the stats and the bitmaps against a recount
    std::vector<Bytes> f;
    for (Bytes n : needles) {
        for (auto &b : n) b = fold1(b, fold);
        f.push_back(n);
    }
    std::sort(f.begin(), f.end());
    f.erase(std::unique(f.begin(), f.end()), f.end());
    uint64_t one = 0, two = 0, blob = 0, every = 0;
    for (const Bytes &n : f) {
        if (n.empty()) every = 1;
        else if (n.size() == 1) ++one;
        else if (n.size() == 2) ++two;
        else blob += n.size();
    }
    ++g_checks;
    if (t.distinct != f.size() || t.one_byte != one || t.two_byte != two || t.blob.size() != blob || t.every != every ||
        t.needles != needles.size() || t.bucket[ss::kSetKeys] != t.entry.size() || t.entry.size() != f.size() - every - one - two) {
        ++g_failures;
        std::printf("FAIL stats\n");
    }
    for (uint32_t k = 0; k < ss::kSetKeys; ++k) {
        const uint32_t bits = ss::set_key_bits(t.bp.data(), k), n = t.bucket[k + 1] - t.bucket[k];
        if (((bits & 2u) != 0) != (n != 0) || n > t.largest_bucket) {
            ++g_failures;
            std::printf("FAIL bucket of key %u\n", k);
        }
        for (uint32_t e = t.bucket[k]; e < t.bucket[k + 1]; ++e) {
            const ss::SetEntry &en = t.entry[e];
            if (en.len < 3 || (uint64_t)en.off + en.len > t.blob.size() || (t.blob[en.off] | (uint32_t)t.blob[en.off + 1] << 8) != k) {
                ++g_failures;
                std::printf("FAIL entry %u\n", e);
            }
        }
    }
}

static void all_strings(const Bytes &alphabet, size_t most, std::vector<Bytes> *out)
{
    out->push_back(Bytes());
    for (size_t b = 0, e = 1, n = 1; n <= most; ++n) {
        for (size_t k = b; k < e; ++k)
            for (uint8_t c : alphabet) out->push_back((*out)[k] + c);
        b = e;
        e = out->size();
    }
}

static Bytes random_string(const Bytes &alphabet, size_t n)
{
    Bytes s;
    for (size_t i = 0; i < n; ++i) s += alphabet[rnd((uint32_t)alphabet.size())];
    return s;
}

static void small_sets(const Bytes &alphabet, int delim, bool fold)
{
    Bytes with_delim = alphabet;
    if (with_delim.find((uint8_t)delim) == Bytes::npos) with_delim += (uint8_t)delim;
    std::vector<Bytes> short_needles, hays;
    all_strings(alphabet, 3, &short_needles);
    all_strings(with_delim, alphabet.size() == 2 ? 7 : 5, &hays);
    const Bytes around = Bytes(1, alphabet[0]) + Bytes(1, (uint8_t)delim) + alphabet + Bytes((const uint8_t *)"x_", 2);
    SetTables t;
    // every set of one or two needles of 0 .. 3 bytes (the empty needle only sets `every`)
    for (size_t a = 0; a < short_needles.size(); ++a) {
        for (size_t b = a; b < short_needles.size(); b += (alphabet.size() == 2 ? 2 : 7)) {
            const std::vector<Bytes> needles = {short_needles[a], short_needles[b]};
            if (!build(needles, fold, &t)) { ++g_failures; continue; }
            if ((a + b) % 8 == 0) check_tables(t, needles, fold);
            for (size_t h = (a * 7 + b) % 23; h < hays.size(); h += 23) check_view(t, needles, fold, hays[h], delim, around);
        }
    }
    // random sets of up to six needles of 0 .. 7 bytes on random haystacks
    for (int round = 0; round < 250; ++round) {
        std::vector<Bytes> needles;
        for (uint32_t k = 1 + rnd(6); k > 0; --k) needles.push_back(random_string(rnd(4) ? alphabet : with_delim, rnd(8)));
        if (!build(needles, fold, &t)) { ++g_failures; continue; }
        if (round % 8 == 0) check_tables(t, needles, fold);
        for (int h = 0; h < 12; ++h) {
            Bytes hay = random_string(with_delim, rnd(25));
            if (!hay.empty() && rnd(2)) {                       // a needle planted at a random place, also across the end
                const Bytes &n = needles[rnd((uint32_t)needles.size())];
                const size_t at = rnd((uint32_t)hay.size());
                hay = hay.substr(0, at) + n + hay.substr(at);
                if (rnd(4) == 0) hay.resize(hay.size() - rnd((uint32_t)hay.size()));
            }
            check_view(t, needles, fold, hay, delim, around);
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
        needles.push_back(Bytes((const uint8_t *)"q", 1));
        needles.push_back(Bytes((const uint8_t *)"ab", 2));
        SetTables t;
        if (!build(needles, fold, &t)) { ++g_failures; continue; }
        check_tables(t, needles, fold);
        if (t.largest_bucket < 200) { ++g_failures; std::printf("FAIL largest bucket %llu\n", (unsigned long long)t.largest_bucket); }
        for (int h = 0; h < 6; ++h) {
            Bytes hay = random_string(alphabet, 40);
            const Bytes &n = needles[rnd(300)];
            hay += h % 3 == 2 ? n.substr(0, n.size() - 1) : n;                   // (one byte short: no match of this needle)
            if (h % 2) hay += random_string(alphabet, 30);
            if (h == 5) hay[hay.size() / 2] = '\n';
            check_view(t, needles, fold, hay, '\n', Bytes((const uint8_t *)"qa\n", 3));
        }
    }
}

// The byte loop of needles of seven bytes and more, with a letter as the delimiter: needles of 3 .. 12 bytes that hold the delimiter
// letter (in either case) at every index, on haystacks that are the needle itself, the needle with that byte in the other case, all
// lower and all upper case.  With the fold a needle that holds the delimiter after folding matches nothing, wherever the letter sits.
static void letter_delimiters(bool fold)
{
    const int delims[] = {'a', 'A'};
    for (int delim : delims) {
        for (size_t n = 3; n <= 12; ++n) {
            for (size_t at = 0; at < n; ++at) {
                for (int letter : delims) {
                    Bytes nd(n, 'x');
                    nd[at] = (uint8_t)letter;
                    const std::vector<Bytes> needles = {nd, Bytes(n, 'x')};
                    SetTables t;
                    if (!build(needles, fold, &t)) { ++g_failures; continue; }
                    Bytes other = nd, lower = nd, upper = nd;
                    other[at] ^= 0x20;
                    for (auto &b : lower) b |= 0x20;
                    for (auto &b : upper) b &= (uint8_t)~0x20;
                    const Bytes around((const uint8_t *)"xa\nA", 4);
                    for (const Bytes &hay : {nd, other, lower, upper, Bytes((const uint8_t *)"..", 2) + other + Bytes((const uint8_t *)" x", 2)})
                        check_view(t, needles, fold, hay, delim, around);
                }
            }
        }
    }
    // the case in so many words: needle xxxxxxa, haystack xxxxxxA, delimiter 'a', folded - the needle holds the delimiter
    SetTables t;
    const std::vector<Bytes> one = {Bytes((const uint8_t *)"xxxxxxa", 7)};
    const Bytes hay((const uint8_t *)"xxxxxxA", 7);
    ++g_checks;
    if (!build(one, true, &t) || ss::set_match_at(t.view(), hay.data(), hay.size(), 0, 'a', 0)) {
        ++g_failures;
        std::printf("FAIL a folded needle that holds the delimiter at index 6 matched\n");
    }
}

int main()
{
    for (int fold = 0; fold <= 1; ++fold) {
        small_sets(Bytes((const uint8_t *)"ab", 2), '\n', fold != 0);
        small_sets(Bytes((const uint8_t *)"ab", 2), 'a', fold != 0);              // the delimiter is a needle byte
        small_sets(Bytes((const uint8_t *)"aA", 2), '\n', fold != 0);
        small_sets(Bytes((const uint8_t *)"aAb", 3), 'A', fold != 0);             // ... an upper-case one: never folded
        small_sets(Bytes((const uint8_t *)"aA.", 3), 'a', fold != 0);             // ... the fold of a haystack byte
        small_sets(Bytes((const uint8_t *)"a_ ", 3), ' ', fold != 0);
        large_sets(fold != 0);
        letter_delimiters(fold != 0);
    }
    // what construction refuses or records
    SetTables t;
    const std::vector<Bytes> dup = {Bytes((const uint8_t *)"Ab", 2), Bytes((const uint8_t *)"aB", 2), Bytes(), Bytes((const uint8_t *)"abc", 3)};
    if (!build(dup, true, &t) || t.distinct != 3 || t.every != 1 || t.two_byte != 1 || t.keys != 1 || t.largest_bucket != 1 || t.fold != 1) {
        ++g_failures;
        std::printf("FAIL folded duplicates\n");
    }
    if (!build(dup, false, &t) || t.distinct != 4 || t.two_byte != 2 || t.fold != 0) {
        ++g_failures;
        std::printf("FAIL unfolded duplicates\n");
    }
    std::printf("needleset_tables_check: %llu checks, %llu failures\n", g_checks, g_failures);
    return g_failures == 0 ? 0 : 1;
}
