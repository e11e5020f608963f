/* sliceslice_hip_setmatches.h - every occurrence of every needle of a compiled set, in ONE pass over the haystack: a count per
 * needle (a word-frequency table) and the ascending list of (offset, needle) pairs (what aho_corasick::find_overlapping_iter or a
 * post-processor of grep -o -b -f FILE wants).  An OPT-IN component shipped in a library of its own.
 *
 *   libsliceslice_hip_setmatches.so  the needleset library's objects PLUS the occurrence scan
 *                                    (sliceslice-rs_amd/csrc/ss_setmatches.hip): every function of sliceslice_hip_needleset.h and of
 *                                    the headers it includes, and the four below.  Linked INSTEAD of libsliceslice_hip.so; searchers
 *                                    and sets belong to the library that made them.
 *
 * Rank:      the position of a needle in the set's sorted, deduplicated order (ss_needle_set_stats.distinct counts that order).
 *            Bytes compare as unsigned, and a proper prefix sorts before the longer needle.  Duplicates and needles that are equal
 *            after the set's fold share a rank.  All needles that can occur at one offset are prefixes of one another, so their
 *            ranks ascend with their lengths.
 * Rule:      for every distinct needle r, d_counts[r] is what ss_count_device returns for a searcher of that needle on the same
 *            view - where `how` carries the fold or SS_BOUND_WORD, what ss_count_nocase_device / ss_count_bounded_device return
 *            (sliceslice_hip_bounded.h has the occurrence rule).  Occurrences overlap.  A needle longer than `len` gives 0.  Bytes
 *            outside [0, len) are absent, whatever memory holds there.  No delimiter exists in these calls, so a needle that holds
 *            '\n' matches like any other.  *total is the sum of the counts, which is the number of (offset, rank) pairs.
 * Order:     ss_find_all_set_device writes the first min(total, capacity) pairs ordered by offset, then by rank.  Nothing is
 *            written at index `capacity` or beyond.  d_offsets and d_ranks may each be NULL; capacity == 0 means the total only.
 *
 *   ss_needle_set_ranks         ranks[k] = the rank of needle k as given to ss_needle_set_new (`needles` entries, host memory).
 *   ss_count_set_device         d_counts (device, `distinct` entries, overwritten; may be NULL) and *total.  Waits for the stream.
 *   ss_count_set_device_async   the same into device memory: d_counts and d_total, either may be NULL, not both.  Stream-ordered: it
 *                               zeroes its outputs on the stream, needs no scratch beyond them and can be captured into a hipGraph,
 *                               as ss_count_device_async can.
 *   ss_find_all_set_device      the pairs and *total.  Waits for the stream.
 *   how       0 or SS_BOUND_WORD.  SS_BOUND_NOCASE is accepted only when it equals the set's fold, as in the line calls.
 * Refused with SS_ERR_ARGUMENT and a message, nothing written: SS_BOUND_LINE, SS_CONTEXT_INVERT and unknown bits in `how`; a
 * mismatch of SS_BOUND_NOCASE with the set's fold; a set that holds the empty needle (out of scope here as in
 * sliceslice_hip_bounded.h: its len + 1 pairs per call belong to no scan); a NULL set; a NULL haystack with len > 0; a NULL total;
 * a set made on another device than the current one; a capturing stream, for the two calls that wait.  The waiting calls take
 * their scratch from a per-call free list and return it on every way out.
 *
 * Cost: the count is ONE scan of the haystack (set_all_kernel: set_scan_kernel's geometry and bitmap lookup; every candidate is
 * walked to the end of its bucket, the bytes behind its key read from memory).  Counts go to a workgroup-private histogram of 4,096
 * bins in LDS - the one-byte and two-byte needles first, then the longer ones by ascending length - flushed with one 64-bit add
 * per non-zero bin and workgroup; a needle without a bin costs one 64-bit device-scope add per occurrence.  Integer adds commute:
 * the output is deterministic.  Find adds the prefix over one word per workgroup and an emit pass over the workgroups that hold one
 * of the first `capacity` pairs; no sort.  Design and measurements: DESIGN.md 5.15.
 *
 * Out of scope: the empty needle; SS_BOUND_LINE and inverted forms; leftmost-longest / non-overlapping selection (it follows on
 * the host from the ordered pairs); batched, plan, sharded, service and host / file forms.  (The non-overlapping occurrences of ONE
 * needle are sliceslice_hip_disjoint.h's; its primitive takes one length, so it does not select among a set's pairs.)
 * (That selection on the device, and a replace with a text per needle: sliceslice_hip_leftmost.h.)
 */
#ifndef SLICESLICE_HIP_SETMATCHES_H
#define SLICESLICE_HIP_SETMATCHES_H

#include "sliceslice_hip_needleset.h"

#ifdef __cplusplus
extern "C" {
#endif

SS_API int ss_needle_set_ranks(const ss_needle_set *set, uint32_t *ranks);
SS_API int ss_count_set_device(const ss_needle_set *set, const void *d_haystack, size_t len, unsigned how, void *hip_stream,
                               uint64_t *d_counts, uint64_t *total);
SS_API int ss_count_set_device_async(const ss_needle_set *set, const void *d_haystack, size_t len, unsigned how, void *hip_stream,
                                     uint64_t *d_counts, uint64_t *d_total);
SS_API int ss_find_all_set_device(const ss_needle_set *set, const void *d_haystack, size_t len, unsigned how, void *hip_stream,
                                  uint64_t *d_offsets, uint32_t *d_ranks, uint64_t capacity, uint64_t *total);

#ifdef __cplusplus
}
#endif
#endif /* SLICESLICE_HIP_SETMATCHES_H */
