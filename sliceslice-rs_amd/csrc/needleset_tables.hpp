// needleset_tables.hpp - the compiled needle set of include/sliceslice_hip_needleset.h: its tables, how they are built (host) and
// how a position of the haystack is looked up in them (host and device, the same text).  Plain C++ without HIP headers, so that a
// host program can run it (tests/native/needleset_tables_check.cpp).
//
// The needles are folded (SS_SET_NOCASE: 'A'..'Z' -> 'a'..'z'), sorted and deduplicated.  Then
//   B1      256 bits: the one-byte needles.  A hit is a match; only the bound test remains.
//   B2, P   65,536 bits each, INTERLEAVED in one array of 4,096 dwords (16 KiB, what a workgroup stages in LDS): key k =
//           first byte | second byte << 8 has B2 at bit 2 * (k & 15) of dword k >> 4 and P one bit above, so that ONE load answers
//           both.  B2: the two-byte needles, a hit is a match.  P: the first two bytes of every needle of three bytes or more.
//   bucket  65,537 indices: the entries of key k are entry[bucket[k] .. bucket[k + 1]), sorted by the needles' bytes.
//   entry   {blob offset, length, bytes 2 .. 5 of the needle as a little-endian dword, the mask of those that exist}: the check of up
//           to four following bytes is one masked dword compare; only needles of seven bytes and more reach the byte loop.
//   every   the set holds the empty needle: every line is selected, nothing is looked up.
// A haystack byte is DEAD for every needle when it is the delimiter - raw, or after the fold (the delimiter itself is never
// folded: a needle byte equal to it is a needle that holds the delimiter, and such a needle matches nothing).  An occurrence
// holds no dead byte and ends at or before `len`; WORD / LINE look at the two neighbours as sliceslice_hip_bounded.h says.
//
// Needle identity (include/sliceslice_hip_setmatches.h): the RANK of a needle is its position in the sorted, deduplicated order -
// bytes compare as unsigned, a proper prefix sorts before the longer needle.  All needles that can occur at one offset are prefixes
// of one another, so their ranks ascend with their lengths, and a bucket's matching entries come in rank order.  Side tables
// (SetRanks), none of them part of SetView:
//   rank_of 1 per needle as given (host only); duplicates and fold-equal needles share a rank
//   rank1   256: the rank of each one-byte needle            erank   the rank of every SetEntry, a parallel array
//   key2, rank2   the two-byte needles' keys, ascending, and their ranks: a B2 hit is a match, so a binary search finds the rank
//   slot    per rank: its bin among the kSetHotSlots bins of a workgroup's histogram, or kSetNoSlot; hot[slot] is the rank again.
//           One-byte and two-byte needles come first, then the longer ones in ascending length, until the bins are full.
// set_each_at reports EVERY needle that occurs at a position, in ascending rank; it knows no delimiter.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <utility>
#include <vector>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SS_SET_HD __host__ __device__ inline
#else
#define SS_SET_HD inline
#endif

namespace ss {

constexpr uint32_t kSetWord = 1u, kSetLine = 2u;        // SS_BOUND_WORD, SS_BOUND_LINE
constexpr uint32_t kSetKeys = 65536u;
constexpr uint32_t kSetBpWords = kSetKeys / 16;         // B2 and P interleaved, two bits per key

struct SetEntry {
    uint32_t off, len;          // the needle: blob[off, off + len), len >= 3
    uint32_t word, mask;        // its bytes 2 .. 5 (those below len) and 0xFF for each of them
};

// The tables as a lookup sees them: pointers into host or into device memory.
struct SetView {
    const uint32_t *b1;         // 8 dwords
    const uint32_t *bp;         // kSetBpWords dwords
    const uint32_t *bucket;     // kSetKeys + 1
    const SetEntry *entry;
    const uint8_t *blob;
    uint32_t fold;              // haystack bytes 'A'..'Z' compare as 'a'..'z'
    uint32_t has1;              // B1 holds a bit
};

constexpr uint32_t kSetHotSlots = 4096u;                // bins of a workgroup's histogram (setmatches_kernels.hpp)
constexpr uint32_t kSetNoSlot = 0xFFFFFFFFu;
constexpr uint32_t kSetNoDelim = 256u;                  // no byte: set_dead is never true, set_bound_ok is the occurrence rule

// The ranks as a lookup sees them: pointers into host or into device memory.
struct SetRanks {
    const uint32_t *rank1;      // 256
    const uint32_t *key2;       // n2 keys, ascending
    const uint32_t *rank2;      // n2
    const uint32_t *erank;      // one per SetEntry
    const uint32_t *slot;       // one per rank
    const uint32_t *hot;        // nhot ranks: hot[slot[r]] == r
    uint32_t n2, nhot;
};

SS_SET_HD uint8_t set_fold(uint8_t b, uint32_t fold) { return fold && (uint8_t)(b - 'A') < 26 ? (uint8_t)(b | 0x20) : b; }
SS_SET_HD bool set_word_byte(uint8_t b) { return (uint8_t)(b - '0') < 10 || (uint8_t)((b | 0x20) - 'a') < 26 || b == '_'; }
SS_SET_HD bool set_dead(uint8_t raw, uint32_t delim, uint32_t fold) { return raw == delim || set_fold(raw, fold) == delim; }
// the two bits of key k: 1 = B2, 2 = P
SS_SET_HD uint32_t set_key_bits(const uint32_t *bp, uint32_t k) { return (bp[k >> 4] >> (2 * (k & 15))) & 3u; }
SS_SET_HD uint32_t set_b1_bit(const uint32_t *b1, uint32_t b) { return (b1[b >> 5] >> (b & 31)) & 1u; }

// the neighbours of hay[g, g + n) in the view [0, len): absent, the delimiter, or (WORD) no word byte
SS_SET_HD bool set_bound_ok(const uint8_t *hay, uint64_t len, uint64_t g, uint64_t n, uint32_t delim, uint32_t how)
{
    if ((how & (kSetWord | kSetLine)) == 0) return true;
    const bool word = (how & kSetWord) != 0;
    if (g > 0) {
        const uint8_t b = hay[g - 1];
        if (b != delim && !(word && !set_word_byte(b))) return false;
    }
    if (g + n < len) {
        const uint8_t b = hay[g + n];
        if (b != delim && !(word && !set_word_byte(b))) return false;
    }
    return true;
}

// The walk through the bucket of `key` for an occurrence at g: hay[g], hay[g + 1] are alive, form the key, and P holds it.
SS_SET_HD bool set_walk(const SetView &v, const uint8_t *hay, uint64_t len, uint64_t g, uint32_t key, uint32_t delim, uint32_t how)
{
    // up to four bytes behind the key, folded; `alive` = 0xFF for each that lies in the view and is not dead
    uint32_t w = 0, alive = 0;
    for (uint32_t k = 0; k < 4; ++k) {
        if (g + 2 + k >= len) break;
        const uint8_t raw = hay[g + 2 + k];
        if (set_dead(raw, delim, v.fold)) break;
        w |= (uint32_t)set_fold(raw, v.fold) << (8 * k);
        alive |= 0xFFu << (8 * k);
    }
    const uint32_t e1 = v.bucket[key + 1];
    for (uint32_t e = v.bucket[key]; e < e1; ++e) {
        const SetEntry en = v.entry[e];
        if ((en.mask & ~alive) != 0 || ((w ^ en.word) & en.mask) != 0) continue;
        if (en.len > 6) {
            if (en.len > len - g) continue;
            const uint8_t *nd = v.blob + en.off;
            uint32_t k = 6;
            for (; k < en.len; ++k) {
                const uint8_t raw = hay[g + k];
                if (set_dead(raw, delim, v.fold) || set_fold(raw, v.fold) != nd[k]) break;
            }
            if (k < en.len) continue;
        }
        if (set_bound_ok(hay, len, g, en.len, delim, how)) return true;
    }
    return false;
}

// Does a needle of the set (the empty one aside) occur at g < len and pass the bound?  Everything from memory: the reference form of
// the lookup, and what the kernels call for a candidate when a bound is asked for.
SS_SET_HD bool set_match_at(const SetView &v, const uint8_t *hay, uint64_t len, uint64_t g, uint32_t delim, uint32_t how)
{
    const uint8_t r0 = hay[g];
    if (set_dead(r0, delim, v.fold)) return false;
    const uint32_t f0 = set_fold(r0, v.fold);
    if (v.has1 && set_b1_bit(v.b1, f0) && set_bound_ok(hay, len, g, 1, delim, how)) return true;
    if (g + 1 >= len) return false;
    const uint8_t r1 = hay[g + 1];
    if (set_dead(r1, delim, v.fold)) return false;
    const uint32_t key = f0 | (uint32_t)set_fold(r1, v.fold) << 8;
    const uint32_t bits = set_key_bits(v.bp, key);
    if ((bits & 1u) && set_bound_ok(hay, len, g, 2, delim, how)) return true;
    return (bits & 2u) && set_walk(v, hay, len, g, key, delim, how);
}

// the rank of the two-byte needle of `key` (B2 holds the key)
SS_SET_HD uint32_t set_rank2(const SetRanks &r, uint32_t key)
{
    uint32_t lo = 0, hi = r.n2;
    while (lo + 1 < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (r.key2[mid] <= key) lo = mid;
        else hi = mid;
    }
    return r.rank2[lo];
}

// EVERY needle of the set (the empty one aside) that occurs at g < len and passes the bound (how: 0 or kSetWord), in ascending
// rank: fn(rank) once per needle.  No delimiter: set_match_at with kSetNoDelim, walked to the end of the bucket.
template <class Fn>
SS_SET_HD void set_each_at(const SetView &v, const SetRanks &r, const uint8_t *hay, uint64_t len, uint64_t g, uint32_t how, Fn &&fn)
{
    const uint32_t f0 = set_fold(hay[g], v.fold);
    if (v.has1 && set_b1_bit(v.b1, f0) && set_bound_ok(hay, len, g, 1, kSetNoDelim, how)) fn(r.rank1[f0]);
    if (g + 1 >= len) return;
    const uint32_t key = f0 | (uint32_t)set_fold(hay[g + 1], v.fold) << 8;
    const uint32_t bits = set_key_bits(v.bp, key);
    if ((bits & 1u) && set_bound_ok(hay, len, g, 2, kSetNoDelim, how)) fn(set_rank2(r, key));
    if ((bits & 2u) == 0) return;
    // up to four bytes behind the key, folded; `alive` = 0xFF for each that lies in the view (set_walk)
    uint32_t w = 0, alive = 0;
    for (uint32_t k = 0; k < 4; ++k) {
        if (g + 2 + k >= len) break;
        w |= (uint32_t)set_fold(hay[g + 2 + k], v.fold) << (8 * k);
        alive |= 0xFFu << (8 * k);
    }
    const uint32_t e1 = v.bucket[key + 1];
    for (uint32_t e = v.bucket[key]; e < e1; ++e) {
        const SetEntry en = v.entry[e];
        if ((en.mask & ~alive) != 0 || ((w ^ en.word) & en.mask) != 0) continue;
        if (en.len > 6) {
            if (en.len > len - g) continue;
            const uint8_t *nd = v.blob + en.off;
            uint32_t k = 6;
            for (; k < en.len; ++k)
                if (set_fold(hay[g + k], v.fold) != nd[k]) break;
            if (k < en.len) continue;
        }
        if (set_bound_ok(hay, len, g, en.len, kSetNoDelim, how)) fn(r.erank[e]);
    }
}

// ---- construction (host) ---------------------------------------------------------------------------------------------------

struct SetTables {
    std::vector<uint32_t> b1, bp, bucket;
    std::vector<SetEntry> entry;
    std::vector<uint8_t> blob;
    uint32_t fold = 0, every = 0;
    // what ss_needle_set_info reports
    uint64_t needles = 0, distinct = 0, one_byte = 0, two_byte = 0, keys = 0, largest_bucket = 0;
    // needle identity (SetRanks)
    std::vector<uint32_t> rank_of, rank1, key2, rank2, erank, slot, hot;

    SetView view() const
    {
        return SetView{b1.data(), bp.data(), bucket.data(), entry.data(), blob.data(), fold, one_byte != 0 ? 1u : 0u};
    }
    SetRanks ranks() const
    {
        return SetRanks{rank1.data(), key2.data(), rank2.data(), erank.data(), slot.data(), hot.data(), (uint32_t)key2.size(), (uint32_t)hot.size()};
    }
};

constexpr int kSetBuilt = 0, kSetBlobTooLarge = 1;

// needles[k] may be null where lens[k] == 0.  Returns kSetBlobTooLarge when the distinct needles hold 2^32 bytes or more (offsets and
// lengths are 32-bit); ss_needle_set_new refuses that earlier, on the sum of the lengths as given, so only other callers can see it.
inline int set_build(const void *const *needles, const size_t *lens, uint32_t count, bool fold, SetTables *t)
{
    *t = SetTables();
    t->fold = fold ? 1u : 0u;
    t->needles = count;
    t->b1.assign(8, 0);
    t->bp.assign(kSetBpWords, 0);
    t->bucket.assign((size_t)kSetKeys + 1, 0);
    // the folded needles, one behind the other
    std::vector<uint64_t> at((size_t)count + 1, 0);
    for (uint32_t k = 0; k < count; ++k) at[k + 1] = at[k] + lens[k];
    std::vector<uint8_t> all((size_t)at[count]);
    for (uint32_t k = 0; k < count; ++k) {
        const uint8_t *src = static_cast<const uint8_t *>(needles[k]);
        for (size_t i = 0; i < lens[k]; ++i) all[(size_t)at[k] + i] = set_fold(src[i], t->fold);
    }
    auto less = [&](uint32_t a, uint32_t b) {
        const size_t la = lens[a], lb = lens[b], m = la < lb ? la : lb;
        const int c = m ? std::memcmp(all.data() + at[a], all.data() + at[b], m) : 0;
        return c != 0 ? c < 0 : la < lb;
    };
    auto same = [&](uint32_t a, uint32_t b) {
        return lens[a] == lens[b] && (lens[a] == 0 || std::memcmp(all.data() + at[a], all.data() + at[b], lens[a]) == 0);
    };
    std::vector<uint32_t> order(count);
    for (uint32_t k = 0; k < count; ++k) order[k] = k;
    std::sort(order.begin(), order.end(), less);
    t->rank_of.assign(count, 0);
    for (uint32_t i = 0, rank = 0; i < count; ++i) {
        if (i != 0 && !same(order[i - 1], order[i])) ++rank;
        t->rank_of[order[i]] = rank;
    }
    order.erase(std::unique(order.begin(), order.end(), same), order.end());
    t->distinct = order.size();
    uint64_t bytes = 0;
    for (uint32_t k : order) bytes += lens[k];
    if (bytes >= (1ull << 32)) return kSetBlobTooLarge;
    t->blob.reserve((size_t)bytes);
    // sorted by bytes means sorted by key FIRST BYTE first; the buckets want the key's numeric order (second byte high), so count,
    // prefix and place
    std::vector<uint32_t> long_ones;
    t->rank1.assign(256, kSetNoSlot);
    std::vector<std::pair<uint32_t, uint32_t>> twos;             // (key, rank)
    for (uint32_t k : order) {
        const uint8_t *nd = all.data() + at[k];
        const size_t n = lens[k];
        if (n == 0) {
            t->every = 1;
        } else if (n == 1) {
            t->b1[nd[0] >> 5] |= 1u << (nd[0] & 31);
            t->rank1[nd[0]] = t->rank_of[k];
            ++t->one_byte;
        } else {
            const uint32_t key = nd[0] | (uint32_t)nd[1] << 8;
            if (n == 2) {
                t->bp[key >> 4] |= 1u << (2 * (key & 15));
                twos.push_back(std::make_pair(key, t->rank_of[k]));
                ++t->two_byte;
            } else {
                t->bp[key >> 4] |= 2u << (2 * (key & 15));
                ++t->bucket[key + 1];
                long_ones.push_back(k);
            }
        }
    }
    for (uint32_t key = 0; key < kSetKeys; ++key) {
        if (t->bucket[key + 1] != 0) ++t->keys;
        if (t->bucket[key + 1] > t->largest_bucket) t->largest_bucket = t->bucket[key + 1];
        t->bucket[key + 1] += t->bucket[key];
    }
    t->entry.resize(long_ones.size());
    t->erank.resize(long_ones.size());
    std::vector<uint32_t> next(t->bucket.begin(), t->bucket.end() - 1);
    for (uint32_t k : long_ones) {                              // (in sorted order: a bucket's entries stay sorted)
        const uint8_t *nd = all.data() + at[k];
        const size_t n = lens[k];
        SetEntry en = {(uint32_t)t->blob.size(), (uint32_t)n, 0, 0};
        for (size_t i = 2; i < n && i < 6; ++i) {
            en.word |= (uint32_t)nd[i] << (8 * (i - 2));
            en.mask |= 0xFFu << (8 * (i - 2));
        }
        t->blob.insert(t->blob.end(), nd, nd + n);
        const uint32_t e = next[nd[0] | (uint32_t)nd[1] << 8]++;
        t->entry[e] = en;
        t->erank[e] = t->rank_of[k];
    }
    std::sort(twos.begin(), twos.end());
    for (const auto &kr : twos) {
        t->key2.push_back(kr.first);
        t->rank2.push_back(kr.second);
    }
    // the hot slots: one-byte needles, two-byte needles, then the longer ones by ascending length (ties in rank order)
    t->slot.assign(order.size(), kSetNoSlot);
    for (uint32_t b = 0; b < 256; ++b)
        if (t->rank1[b] != kSetNoSlot) t->hot.push_back(t->rank1[b]);
    t->hot.insert(t->hot.end(), t->rank2.begin(), t->rank2.end());
    std::stable_sort(long_ones.begin(), long_ones.end(), [&](uint32_t a, uint32_t b) { return lens[a] < lens[b]; });
    for (uint32_t k : long_ones) t->hot.push_back(t->rank_of[k]);
    if (t->hot.size() > kSetHotSlots) t->hot.resize(kSetHotSlots);
    for (uint32_t s = 0; s < t->hot.size(); ++s) t->slot[t->hot[s]] = s;
    return kSetBuilt;
}

}  // namespace ss
