/* sliceslice_hip_matches_batched.h - every occurrence of MANY needles in MANY haystacks in one call: per-problem counts, and
 * per-problem offsets in CSR form.  The batched form of sliceslice_hip_matches.h, as ss_search_batched / ss_find_batched are the
 * batched forms of ss_search_device / ss_find_device.  An OPT-IN component shipped in a library of its own:
 *
 *   libsliceslice_hip.so                  the drop-in library: every function of sliceslice_hip.h
 *   libsliceslice_hip_matches.so          the same objects plus the three functions of sliceslice_hip_matches.h
 *   libsliceslice_hip_matches_batched.so  the matches library's objects plus ss_matches_batched.hip and scan_inst_all_batched.hip
 *                                         (sliceslice-rs_amd/csrc): every function of the two headers above and the two below
 *
 * A process uses ONE of them (searchers belong to the library that made them).
 *
 * Problems are given as range arrays exactly as in ss_search_batched: problem i is the needle
 * d_needles[needle_begin[i] .. needle_end[i]) in the haystack d_haystacks[hay_begin[i] .. hay_end[i]); everything lives in device
 * memory, the four range arrays hold `count` uint64 each, CSR callers pass (off, off + 1), and ranges may alias (4,585 needles
 * against ONE haystack).  Every problem takes the `new` rule (there is no `position` argument, as in ss_find_batched).
 *
 * Match rules of the single calls: OVERLAPPING occurrences - every offset k with haystack_i[k .. k + n_i) == needle_i; the empty
 * needle matches at 0 .. len_i (len_i + 1 times); n_i > len_i: 0.  Offsets are relative to the problem's OWN haystack start
 * (hay_begin[i]), 64-bit, as ss_find_batched reports them.
 *
 * Argument checks, error codes and ss_last_error follow ss_search_batched; count == 0 is valid.  Like the single calls, these
 * neither start nor read any tuning: the filter bytes are chosen by the STATIC byte classes, the calls do not enter the
 * remembered batches of ss_search_batched and sample no histogram, so no answer and no launch depends on an earlier call.  All
 * scratch is owned by the call (two threads on two streams never share any).
 *
 * THE GRID.  The haystack lengths live on the device, and neither call reads them back to size its launch (ss_find_all_batched
 * waits for its stream anyway, but sizes its grid by the same rule: one code path, one set of descriptors for both passes).  The
 * grid holds 96 workgroups per CU - 24,576 on 256 CUs - shared out evenly: slices = ceil(24,576 / count) workgroups per problem,
 * each scanning a contiguous run of its problem's 16 KiB tiles; count x slices <= 2^31 - 1.  From 24,576 problems on there is
 * ONE workgroup per problem, and since nothing exits early, a single very long problem among them is scanned by that one
 * workgroup alone, at some 2.2 us per tile: 256 MiB take 36 ms.  Batches of a few long problems get many slices each and run at
 * the rate of the single calls.
 *
 *   ss_count_batched      d_counts[i] = occurrences of needle i in haystack i.  Stream-ordered, no host wait; d_counts (count
 *                         uint64, device memory) needs no initialisation.  Not capturable into a hipGraph (SS_ERR_ARGUMENT on a
 *                         capturing stream, as ss_search_batched: the call's scratch goes back to a free list that later calls
 *                         take from).
 *   ss_find_all_batched   CSR.  d_row_begin[i] = sum of the counts of problems < i (count + 1 entries; d_row_begin[count] = the
 *                         total); d_offsets[d_row_begin[i] .. d_row_begin[i + 1]) = problem i's offsets, ascending.  Only ranks
 *                         below `capacity` are written - the leftmost min(total, capacity) in (problem, offset) order;
 *                         d_offsets[capacity ..] is never touched; capacity == 0 (d_offsets may be NULL): rows and counts only.
 *                         d_counts may be NULL.  Waits for the stream; *total = d_row_begin[count].
 */
#ifndef SLICESLICE_HIP_MATCHES_BATCHED_H
#define SLICESLICE_HIP_MATCHES_BATCHED_H

#include "sliceslice_hip_matches.h"

#ifdef __cplusplus
extern "C" {
#endif

SS_API int ss_count_batched(const void *d_haystacks, const uint64_t *d_hay_begin, const uint64_t *d_hay_end,
                            const void *d_needles, const uint64_t *d_needle_begin, const uint64_t *d_needle_end,
                            size_t count, void *hip_stream, uint64_t *d_counts);
SS_API int ss_find_all_batched(const void *d_haystacks, const uint64_t *d_hay_begin, const uint64_t *d_hay_end,
                               const void *d_needles, const uint64_t *d_needle_begin, const uint64_t *d_needle_end,
                               size_t count, void *hip_stream, uint64_t *d_counts, uint64_t *d_row_begin,
                               uint64_t *d_offsets, uint64_t capacity, uint64_t *total);

#ifdef __cplusplus
}
#endif
#endif /* SLICESLICE_HIP_MATCHES_BATCHED_H */
