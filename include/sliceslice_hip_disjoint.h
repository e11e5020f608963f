/* sliceslice_hip_disjoint.h - the NON-OVERLAPPING occurrences of a needle: how many, where, and the haystack with each of them
 * replaced (Python's bytes.count and bytes.replace, Rust's str::matches, memmem::find_iter and str::replace, grep -o,
 * sed 's/needle/text/g').  An OPT-IN component shipped in a library of its own.
 *
 *   libsliceslice_hip_disjoint.so  the setmatches library's objects PLUS the selection and the replace kernels
 *                                  (sliceslice-rs_amd/csrc/ss_disjoint.hip): every function of sliceslice_hip_setmatches.h and of
 *                                  the headers it includes, and the five below.  Linked INSTEAD of libsliceslice_hip.so; searchers
 *                                  belong to the library that made them.
 *
 * Rule:      the occurrences are those that the model call for `how` keeps, in ascending order:
 *              how == 0                                          ss_find_all_device
 *              how == SS_BOUND_NOCASE                            ss_find_all_nocase_device
 *              SS_BOUND_WORD, alone or with SS_BOUND_NOCASE      ss_find_all_bounded_device
 *            The first occurrence is selected.  After a selected occurrence at p, the next selected one is the first occurrence at
 *            or beyond p + n (n: the needle's length).  The bounds test comes before the selection: an occurrence that is not a
 *            whole word neither is selected nor blocks a later one.  "aa" in "aaaa": 2, at 0 and 2.  GNU grep -o -b -w -F and
 *            Python's re.finditer with two lookarounds agree ("aa" in "aaa aa -aa-aa- aa": 4, 8, 11, 15).  Bytes outside [0, len)
 *            are absent, whatever memory holds there.  Everything is 64-bit.
 * Empty needle: with how == 0 the count and find calls give the model's len + 1 offsets, since nothing overlaps; the replace call
 *            refuses it.
 *
 *   ss_select_disjoint_device    the primitive: the greedy selection over a list of offsets.  `s` names the device and scratch
 *                                only.  d_offsets[0, count) are strictly ascending; that is the caller's contract.  n >= 1 is any
 *                                64-bit length.  *selected is the size of the greedy selection; the leftmost
 *                                min(total, capacity) selected offsets are written ascending.  Nothing is written at index
 *                                `capacity` or beyond.  capacity == 0 or a NULL d_selected means count only; count == 0 gives 0
 *                                with no launch.  On a breach of the ordering contract nothing faults and nothing is written
 *                                outside the first min(total, capacity) entries; the values are then unspecified.  The primitive
 *                                takes one length: leftmost-longest selection over a needle set's (offset, rank) pairs is out of
 *                                scope.  Waits for the stream.
 *   ss_count_disjoint_device     *count = the number of selected occurrences.  Waits for the stream.
 *   ss_find_all_disjoint_device  *count = that number; d_offsets[0 .. min(count, capacity)) = the leftmost selected offsets,
 *                                ascending; capacity == 0 (d_offsets may be NULL): count only.  Waits for the stream.
 *   ss_replace_device            `replacement` is host memory, replacement_len may be 0.  *count is the disjoint count and
 *                                *out_len = len + count * (replacement_len - n), computed in 64 bits.  If out_capacity < *out_len,
 *                                nothing is written and the call returns SS_OK: the caller sizes the buffer and calls again.
 *                                Otherwise d_out[0, *out_len) equals bytes.replace(needle, replacement) of the view, and nothing
 *                                is written at *out_len or beyond.  Waits for the stream.
 * Refused with SS_ERR_ARGUMENT and a message that says why, nothing written: SS_BOUND_LINE, SS_CONTEXT_INVERT and unknown bits in
 * `how`; the empty needle with any `how` bit, and in ss_replace_device; a capturing stream; NULL result pointers; n == 0,
 * d_selected == d_offsets, a NULL d_offsets with count > 0 and 2^48 or more offsets in the primitive; an overflow of *out_len, a
 * NULL replacement with replacement_len > 0 and a d_out range that intersects the haystack's range in ss_replace_device.
 * Everything else the model call refuses is refused by it, with its message.
 *
 * Cost: the host computes the needle's longest proper border (the longest proper prefix that is also a suffix; of the folded
 * needle where `how` has SS_BOUND_NOCASE).  Border 0 - nearly every real needle - means no two occurrences can overlap: the call IS
 * the model call, the same launches, no temporary memory.  Border above 0: the model's count gives M; M == 0 ends the call;
 * otherwise the model's find call runs into temporary device memory of 8 bytes per overlapping occurrence (the precedent of
 * ss_find_lines_context_device), the primitive runs on that list with scratch of another 8 bytes per offset, and the memory is
 * returned inside the call.  A failed allocation returns SS_ERR_NOMEM or SS_ERR_HIP with nothing written.  The selection works on
 * blocks of SS_DISJOINT_BLOCK offsets staged in LDS: a chain re-synchronises at every run head (an offset n or more beyond its
 * predecessor), and the successor of entry j has index at most j + n.  No workgroup waits for another, no global atomic, the
 * output is deterministic.  ss_replace_device reads the haystack in parts of SS_CONTEXT_PART_BYTES and writes every output byte
 * exactly once.  Design and measurements: DESIGN.md 5.16.
 *
 * Out of scope: leftmost-longest selection over a needle set's pairs; SS_BOUND_LINE and inverted forms; an async / capturable
 * form; batched, plan, sharded, service and host / file forms; regular expressions and back-references in the replacement.
 * (Leftmost-longest selection over a set's pairs, and a replace with a text per needle: sliceslice_hip_leftmost.h.)
 */
#ifndef SLICESLICE_HIP_DISJOINT_H
#define SLICESLICE_HIP_DISJOINT_H

#include "sliceslice_hip_setmatches.h"

#define SS_DISJOINT_BLOCK 4096u     /* offsets per workgroup of the selection kernels */

#ifdef __cplusplus
extern "C" {
#endif

SS_API int ss_select_disjoint_device(const ss_searcher *s, const uint64_t *d_offsets, uint64_t count, uint64_t n, void *hip_stream,
                                     uint64_t *d_selected, uint64_t capacity, uint64_t *selected);
SS_API int ss_count_disjoint_device(const ss_searcher *s, const void *d_haystack, size_t len, unsigned how, void *hip_stream,
                                    uint64_t *count);
SS_API int ss_find_all_disjoint_device(const ss_searcher *s, const void *d_haystack, size_t len, unsigned how, void *hip_stream,
                                       uint64_t *d_offsets, uint64_t capacity, uint64_t *count);
SS_API int ss_replace_device(const ss_searcher *s, const void *d_haystack, size_t len, unsigned how, const void *replacement,
                             size_t replacement_len, void *hip_stream, void *d_out, uint64_t out_capacity, uint64_t *out_len,
                             uint64_t *count);

#ifdef __cplusplus
}
#endif
#endif /* SLICESLICE_HIP_DISJOINT_H */
