// disjoint_host.hpp - what the host knows about non-overlapping occurrences (include/sliceslice_hip_disjoint.h): the needle's
// longest proper border, which decides whether two occurrences can overlap at all, and the greedy walk itself, the rule the
// selection kernels (disjoint_kernels.hpp) implement.  Host-only and free of HIP, so that a stand-alone program can sweep it
// (tests/native/disjoint_host_check.cpp); nothing here is exported.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace ssh {

// The length of the longest proper prefix of needle[0, n) that is also its suffix (the last value of the Knuth-Morris-Pratt failure
// function).  Two occurrences of the needle can overlap - stand less than n apart - if and only if it is above 0.
inline size_t longest_proper_border(const uint8_t *needle, size_t n)
{
    if (n < 2) return 0;
    std::vector<size_t> fail(n, 0);
    size_t k = 0;
    for (size_t i = 1; i < n; ++i) {
        while (k > 0 && needle[i] != needle[k]) k = fail[k - 1];
        if (needle[i] == needle[k]) ++k;
        fail[i] = k;
    }
    return fail[n - 1];
}

// The greedy selection over strictly ascending offsets: the first is selected; after a selected p the next selected one is the first
// at or beyond p + n.  Writes the leftmost min(total, capacity) selected offsets (out may be NULL) and returns the total.
inline uint64_t select_disjoint_host(const uint64_t *offsets, uint64_t count, uint64_t n, uint64_t *out, uint64_t capacity)
{
    uint64_t total = 0, next = 0;
    bool any = false;
    for (uint64_t j = 0; j < count; ++j) {
        if (any && offsets[j] < next) continue;
        if (out && total < capacity) out[total] = offsets[j];
        ++total;
        any = true;
        if (offsets[j] > UINT64_MAX - n) break;                 // (nothing can stand at or beyond p + n)
        next = offsets[j] + n;
    }
    return total;
}

// *out_len = len + count * (replacement_len - n) in 64 bits; false on overflow.  count * n <= len holds for a disjoint count.
inline bool replaced_length(uint64_t len, uint64_t count, uint64_t n, uint64_t replacement_len, uint64_t *out_len)
{
    if (count != 0 && n > len / count) return false;            // (not a disjoint count of this view)
    const uint64_t kept = len - count * n;
    if (count != 0 && replacement_len > (UINT64_MAX - kept) / count) return false;
    *out_len = kept + count * replacement_len;
    return true;
}

}  // namespace ssh
