// anyof_segments_check.cpp - the index arithmetic of the union of ascending lists (sliceslice-rs_amd/csrc/anyof_segments.hpp) on the
// host, against a brute-force union.  A stand-alone program: tests/test_anyof_cpu.py compiles it for the host with
// -fsanitize=address,undefined and runs it as a child process.
//
//   a small segment size (4 numbers): every N <= 10, every subset of 1 .. N split over 1 to 3 lists (every entry in the list its
//   position names, and also in the next one: duplicates across lists), with a 0 and an N + 1 added, with and without complement,
//   every capacity 0 .. total + 1 into a buffer of exactly that size - count, prefix and emit as the kernels do them
//   the real segment size: segment, word and bit of 1, 31, 32, 33, 64, 65, 65,535, 65,536, 65,537, 131,072, 131,073 and 2^64 - 1,
//   the cut of the last segment, the word masks
//   lists out of order (a breach of the caller's contract): every written value stays in 1 .. limit and below the capacity
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../sliceslice-rs_amd/csrc/anyof_segments.hpp"

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

// The kernels' three steps on the host, for segments of L numbers: per segment the bitmap from the lists' slices and its count, the
// exclusive prefix, and the emit pass, which skips a segment at or above the capacity.  `out` has exactly `capacity` elements.
template <uint64_t L>
static uint64_t union_as_the_kernels(const std::vector<uint64_t> &numbers, const std::vector<uint64_t> &off, uint64_t limit, int complement,
                                     std::vector<uint64_t> &out)
{
    using Seg = ss::AnySegments<L>;
    const uint64_t segs = Seg::segments(limit), capacity = out.size(), lists = off.size() - 1;
    std::vector<uint64_t> cnt(segs), pre(segs);
    auto bitmap = [&](uint64_t g) {
        std::vector<uint32_t> bits(Seg::kWords, 0);
        const uint64_t first = Seg::first(g), last = Seg::last(g, limit);
        for (uint64_t k = 0; k < lists; ++k) {
            if (off[k] >= off[k + 1]) continue;
            const ss::AnySlice sl = ss::any_slice(numbers.data(), off[k], off[k + 1], first, last);
            EXPECT(off[k] <= sl.lo && sl.lo <= sl.hi && sl.hi <= off[k + 1], "slice [%llu, %llu) of list [%llu, %llu)", (unsigned long long)sl.lo,
                   (unsigned long long)sl.hi, (unsigned long long)off[k], (unsigned long long)off[k + 1]);
            for (uint64_t i = sl.lo; i < sl.hi; ++i)
                if (ss::any_inside(numbers[i], first, last)) bits.at(Seg::word_of(numbers[i])) |= Seg::bit_of(numbers[i]);
        }
        return bits;
    };
    uint64_t total = 0;
    for (uint64_t g = 0; g < segs; ++g) {
        const std::vector<uint32_t> bits = bitmap(g);
        uint64_t n = 0;
        for (uint32_t w = 0; w < Seg::kWords; ++w) n += ss::any_popc(Seg::out_bits(bits[w], w, Seg::valid(g, limit), complement));
        cnt[g] = n;
        pre[g] = total;
        total += n;
    }
    for (uint64_t g = 0; g < segs; ++g) {
        if (pre[g] >= capacity || cnt[g] == 0) continue;
        const std::vector<uint32_t> bits = bitmap(g);
        uint64_t slot = pre[g];
        for (uint32_t w = 0; w < Seg::kWords && slot < capacity; ++w)
            slot = ss::any_emit_word(Seg::out_bits(bits[w], w, Seg::valid(g, limit), complement), Seg::number_at(g, w, 0), slot, capacity, out.data());
    }
    return total;
}

template <uint64_t L>
static void sweep(const std::vector<std::vector<uint64_t>> &lists, uint64_t N, int complement)
{
    std::vector<char> in(N + 2, 0);
    std::vector<uint64_t> numbers, off(1, 0);
    for (const auto &l : lists) {
        for (uint64_t v : l) {
            numbers.push_back(v);
            if (v >= 1 && v <= N) in[v] = 1;
        }
        off.push_back(numbers.size());
    }
    std::vector<uint64_t> want;
    for (uint64_t v = 1; v <= N; ++v)
        if ((in[v] != 0) != (complement != 0)) want.push_back(v);
    for (uint64_t capacity = 0; capacity <= want.size() + 1; ++capacity) {
        std::vector<uint64_t> out(capacity, 0);                             // exactly `capacity` elements: ASan sees a write behind them
        const uint64_t total = union_as_the_kernels<L>(numbers, off, N, complement, out);
        EXPECT(total == want.size(), "N %llu complement %d: total %llu, want %zu", (unsigned long long)N, complement, (unsigned long long)total, want.size());
        bool same = true;
        for (uint64_t i = 0; i < capacity; ++i) same = same && out[i] == (i < want.size() ? want[i] : 0);
        EXPECT(same, "N %llu complement %d capacity %llu lists %zu", (unsigned long long)N, complement, (unsigned long long)capacity, lists.size());
    }
}

int main()
{
    constexpr uint64_t kSmall = 4;
    for (uint64_t N = 0; N <= 10; ++N)
        for (uint64_t mask = 0; mask < (1ull << N); ++mask)
            for (uint64_t nl = 1; nl <= 3; ++nl)
                for (int complement = 0; complement < 2; ++complement) {
                    std::vector<std::vector<uint64_t>> lists(nl), twice(nl), wide(nl);
                    uint64_t i = 0;
                    for (uint64_t v = 1; v <= N; ++v) {
                        if (!(mask >> (v - 1) & 1)) continue;
                        lists[i % nl].push_back(v);
                        twice[i % nl].push_back(v);
                        if (nl > 1) twice[(i + 1) % nl].push_back(v);       // the same number in two lists; each list still ascends
                        ++i;
                    }
                    sweep<kSmall>(lists, N, complement);
                    if (nl > 1) sweep<kSmall>(twice, N, complement);
                    for (uint64_t k = 0; k < nl; ++k) {                     // 0 in front, N + 1 behind: still strictly ascending
                        wide[k].push_back(0);
                        wide[k].insert(wide[k].end(), lists[k].begin(), lists[k].end());
                        wide[k].push_back(N + 1);
                    }
                    sweep<kSmall>(wide, N, complement);
                }
    EXPECT(g_checks > 0, "the sweep ran");
    // the real segment size at its borders
    using Seg = ss::AnySegments<65536>;
    struct { uint64_t v, seg; uint32_t word, bit; } at[] = {
        {1, 0, 0, 0}, {31, 0, 0, 30}, {32, 0, 0, 31}, {33, 0, 1, 0}, {64, 0, 1, 31}, {65, 0, 2, 0}, {65535, 0, 2047, 30}, {65536, 0, 2047, 31},
        {65537, 1, 0, 0}, {131072, 1, 2047, 31}, {131073, 2, 0, 0}, {~0ull, (~0ull - 1) / 65536, 2047, 30}};
    EXPECT(Seg::kWords == 2048, "words");
    for (const auto &a : at) {
        EXPECT(Seg::segment_of(a.v) == a.seg && Seg::word_of(a.v) == a.word && Seg::bit_of(a.v) == 1u << a.bit, "number %llu: segment %llu word %u bit 0x%x",
               (unsigned long long)a.v, (unsigned long long)Seg::segment_of(a.v), Seg::word_of(a.v), Seg::bit_of(a.v));
        EXPECT(Seg::number_at(a.seg, a.word, a.bit) == a.v, "number_at of %llu", (unsigned long long)a.v);
        EXPECT(Seg::first(a.seg) <= a.v && a.v <= Seg::last(a.seg, a.v) && Seg::last(a.seg, a.v) == a.v, "first / last of %llu", (unsigned long long)a.v);
        EXPECT(Seg::segments(a.v) == a.seg + 1 && Seg::valid(a.seg, a.v) == (a.v - 1) % 65536 + 1, "segments / valid of limit %llu", (unsigned long long)a.v);
        // as the limit: its own bit is the last one that the cut leaves
        const uint32_t m = Seg::word_mask(a.word, Seg::valid(a.seg, a.v));
        EXPECT((m & (1u << a.bit)) && (a.bit == 31 || !(m >> (a.bit + 1))), "mask of limit %llu: 0x%x", (unsigned long long)a.v, m);
        EXPECT(a.word == 2047 || Seg::word_mask(a.word + 1, Seg::valid(a.seg, a.v)) == 0, "the word behind limit %llu", (unsigned long long)a.v);
        EXPECT(a.word == 0 || Seg::word_mask(a.word - 1, Seg::valid(a.seg, a.v)) == ~0u, "the word in front of limit %llu", (unsigned long long)a.v);
    }
    EXPECT(Seg::segments(0) == 0 && Seg::segments(65536) == 1 && Seg::segments(65537) == 2 && Seg::segments(~0ull) == (1ull << 48), "segments");
    EXPECT(Seg::valid(0, 65536) == 65536 && Seg::valid(1, 65537) == 1 && Seg::valid(0, 200000) == 65536 && Seg::valid(3, 200000) == 200000 - 3 * 65536, "valid");
    EXPECT(Seg::out_bits(0x5u, 0, 3, 0) == 0x5u && Seg::out_bits(0x5u, 0, 3, 1) == 0x2u && Seg::out_bits(0, 2047, 65536, 1) == ~0u, "out_bits");
    {
        uint64_t out[3] = {0, 0, 0};
        EXPECT(ss::any_emit_word(0x80000001u, 100, 1, 2, out) == 3 && out[0] == 0 && out[1] == 100 && out[2] == 0, "emit stops at the capacity");
    }
    // lists out of order: the searches end inside the list, and every written value is a number of 1 .. limit
    const uint64_t breach[][5] = {{5, 3, 9, 1, 7}, {9, 9, 9, 1, 1}, {0, 11, 2, 2, 0}, {10, 8, 6, 4, 2}, {3, 3, 3, 3, 3}};
    for (const auto &b : breach)
        for (int complement = 0; complement < 2; ++complement)
            for (uint64_t capacity = 0; capacity <= 11; ++capacity) {
                std::vector<uint64_t> numbers(b, b + 5), off = {0, 2, 5}, out(capacity, 0);
                const uint64_t total = union_as_the_kernels<kSmall>(numbers, off, 10, complement, out);
                EXPECT(total <= 10, "breach: total %llu", (unsigned long long)total);
                for (uint64_t i = 0; i < capacity; ++i)
                    EXPECT(i < total ? (out[i] >= 1 && out[i] <= 10) : out[i] == 0, "breach: out[%llu] = %llu", (unsigned long long)i, (unsigned long long)out[i]);
            }
    std::printf("%ld checks, %ld failures\n", g_checks, g_failures);
    return g_failures ? 1 : 0;
}
