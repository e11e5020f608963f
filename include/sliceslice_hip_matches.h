/* sliceslice_hip_matches.h - every occurrence of a needle: how many, and where.  An OPT-IN component shipped in a library of its
 * own, like the resident search service.
 *
 *   libsliceslice_hip.so          the drop-in library: every function of sliceslice_hip.h, none of the three below
 *   libsliceslice_hip_matches.so  the same objects PLUS the all-matches scan (sliceslice-rs_amd/csrc/ss_matches.hip,
 *                                 scan_inst_all.hip): every function of sliceslice_hip.h and the three below
 *
 * A process uses ONE of the two: searchers belong to the library that made them, so a handle from one must never be passed to
 * the other.
 *
 * Occurrences are OVERLAPPING: every offset i with haystack[i .. i+n) == needle ("aa" in "aaaa": 3, at 0, 1, 2).
 * Empty needle: len + 1 occurrences at 0 .. len (Python's bytes.count, memchr's find_iter).  n > len: 0.
 * Non-overlapping counts (bytes.count's rule for needles that overlap themselves) follow from the offsets on the host: walk them
 * in order and keep an offset when it is at least n past the last one kept.  (That walk, on the device, and the replacement of the
 * occurrences it keeps are sliceslice_hip_disjoint.h's.)
 *
 * Argument checks, error codes and ss_last_error follow ss_find_device; the calls work for every searcher the constructors and
 * ss_searcher_set_filter3 can make, and offsets are 64-bit (haystacks above 4 GiB included).  The calls neither start nor read the
 * launch tuning of sliceslice_hip.h (the census): a search's tuning state is the same before and after them.
 *
 *   ss_count_device        *count = number of occurrences; waits for the stream.
 *   ss_count_device_async  the same, stream-ordered, no host wait, capturable into a hipGraph: the count lands in *d_count
 *                          (device memory, overwritten).
 *   ss_find_all_device     *count = total number of occurrences; d_offsets[0 .. min(total, capacity)) = the leftmost
 *                          min(total, capacity) offsets in ascending order; d_offsets[capacity ..] is never written.
 *                          capacity == 0 (d_offsets may be NULL): count only.  Waits for the stream.
 */
#ifndef SLICESLICE_HIP_MATCHES_H
#define SLICESLICE_HIP_MATCHES_H

#include "sliceslice_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

SS_API int ss_count_device(const ss_searcher *s, const void *d_haystack, size_t len, void *hip_stream, uint64_t *count);
SS_API int ss_count_device_async(const ss_searcher *s, const void *d_haystack, size_t len, void *hip_stream, uint64_t *d_count);
SS_API int ss_find_all_device(const ss_searcher *s, const void *d_haystack, size_t len, void *hip_stream, uint64_t *d_offsets,
                              uint64_t capacity, uint64_t *count);

#ifdef __cplusplus
}
#endif
#endif /* SLICESLICE_HIP_MATCHES_H */
