// leftmost_host.hpp - what the host knows about leftmost-longest selection and the set replace
// (include/sliceslice_hip_leftmost.h).  Two functions are what ss_leftmost.hip calls: rank_replacements, the replacement that belongs
// to every rank, and replaced_set_length, the output's length with its overflow check.  Two are MODELS that no library code calls -
// the device computes both - kept beside them as the statement of what the kernels must give: select_leftmost_host, the rule of
// the selection kernels written as a loop, and replaced_starts_host, the output offset of every selection.  Host-only and free of
// HIP, so that a stand-alone program can sweep all four (tests/native/leftmost_host_check.cpp); nothing here is exported.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

namespace ssh {

constexpr uint32_t kLeftmostNoNeedle = 0xffffffffu;

// (Model; no library code calls it.)  The selection over entries (offsets[j], lengths[j]), offsets ascending, lengths ascending within a run of equal offsets: the last
// entry of a run is its candidate; the first candidate is selected; after a selected p of length l the next is the first candidate
// at or beyond p + l.  Writes the leftmost min(total, capacity) selected offsets and their indices (each may be NULL); returns the
// total.
inline uint64_t select_leftmost_host(const uint64_t *offsets, const uint64_t *lengths, uint64_t count, uint64_t *out, uint64_t *which,
                                     uint64_t capacity)
{
    uint64_t total = 0, next = 0;
    for (uint64_t j = 0; j < count; ++j) {
        if (j + 1 < count && offsets[j + 1] == offsets[j]) continue;        // (a longer one follows at this offset)
        if (offsets[j] < next) continue;
        if (total < capacity) {
            if (out) out[total] = offsets[j];
            if (which) which[total] = j;
        }
        ++total;
        if (offsets[j] > UINT64_MAX - lengths[j]) break;                    // (nothing can stand at or beyond p + l)
        next = offsets[j] + lengths[j];
    }
    return total;
}

// owner[r] = the first needle as given whose rank is r (kLeftmostNoNeedle: none).  Returns -1, or the index of the first needle
// whose replacement differs from that of the earlier needle of its rank.
inline int64_t rank_replacements(const uint32_t *rank_of, uint32_t needles, const void *const *replacements, const size_t *replacement_lens,
                                 size_t distinct, std::vector<uint32_t> *owner)
{
    owner->assign(distinct, kLeftmostNoNeedle);
    for (uint32_t k = 0; k < needles; ++k) {
        const uint32_t r = rank_of[k];
        if (r >= distinct) return (int64_t)k;
        uint32_t &first = (*owner)[r];
        if (first == kLeftmostNoNeedle) {
            first = k;
        } else if (replacement_lens[first] != replacement_lens[k] ||
                   (replacement_lens[k] != 0 && std::memcmp(replacements[first], replacements[k], replacement_lens[k]) != 0)) {
            return (int64_t)k;
        }
    }
    return -1;
}

// *out_len = len + delta, where delta is the sum over `count` selections of (replacement length - needle length) modulo 2^64.  False
// where count * longest_replacement + len does not fit 64 bits: the true length lies at or below that bound, so below it the
// modular sum IS the length.
inline bool replaced_set_length(uint64_t len, uint64_t count, uint64_t longest_replacement, uint64_t delta, uint64_t *out_len)
{
    if (count != 0 && longest_replacement > (UINT64_MAX - len) / count) return false;
    *out_len = len + delta;
    return true;
}

// (Model; no library code calls it.)  starts[i] = the output offset of selection i's replacement: its offset + the sum of the earlier (replacement - needle) lengths.
// Returns the sum over all of them, modulo 2^64.
inline uint64_t replaced_starts_host(const uint64_t *selected, const uint64_t *needle_lens, const uint64_t *replacement_lens, uint64_t count,
                                     uint64_t *starts)
{
    uint64_t delta = 0;
    for (uint64_t i = 0; i < count; ++i) {
        starts[i] = selected[i] + delta;
        delta += replacement_lens[i] - needle_lens[i];
    }
    return delta;
}

}  // namespace ssh
