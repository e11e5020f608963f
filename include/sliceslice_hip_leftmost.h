/* sliceslice_hip_leftmost.h - the LEFTMOST-LONGEST, non-overlapping occurrences of a compiled needle set: how many, where, which
 * needle, and the haystack with each of them replaced by its needle's own text (grep -o -F -f FILE, aho_corasick's
 * MatchKind::LeftmostLongest find_iter and replace_all, re.sub over an alternation of literals sorted longest first).  An OPT-IN
 * component shipped in a library of its own.
 *
 *   libsliceslice_hip_leftmost.so  the output library's objects PLUS the selection and the set-replace kernels
 *                                  (sliceslice-rs_amd/csrc/ss_leftmost.hip): every function of sliceslice_hip_output.h and of the
 *                                  headers it includes, and the five below.  Linked INSTEAD of libsliceslice_hip.so; searchers and
 *                                  sets belong to the library that made them.
 *
 * Rule:      the occurrences are those ss_find_all_set_device lists for the same set and `how` (0 or SS_BOUND_WORD; SS_BOUND_NOCASE
 *            is accepted only when it equals the set's fold).  Among the pairs at one offset, the one with the greatest rank is
 *            the candidate: ranks ascend with length there, so it is the longest.  The first candidate is selected.  After a
 *            selection at p of length L, the next selected one is the first candidate at or beyond p + L.  The word test comes
 *            before the selection: a candidate that is not a whole word neither is selected nor blocks, and a shorter needle at
 *            the same offset that is a whole word then is the candidate.  {the, then, there, he, here} in "then there here": then
 *            at 0, there at 5, here at 11.  Bytes outside [0, len) are absent, whatever memory holds there.  Everything is 64-bit.
 *            A set that holds the empty needle is refused, as in sliceslice_hip_setmatches.h.
 *
 *   ss_select_leftmost_device       the primitive: the selection over any list of (offset, length) entries.  `set` names the device
 *                                   and its scratch only.  d_offsets[0, count) ascend and may repeat; d_lengths (64-bit, each >= 1)
 *                                   ascend within a run of equal offsets; that is the caller's contract.  *selected is the size of
 *                                   the selection; the leftmost min(total, capacity) selected offsets are written ascending to
 *                                   d_selected and their indices in the input list to d_which.  Either array may be NULL;
 *                                   capacity == 0 means count only.  Nothing is written at index `capacity` or beyond.  count == 0
 *                                   gives 0 with no launch.  On a breach of the contract nothing faults and nothing is written
 *                                   outside the first min(total, capacity) entries; the values are then unspecified.  A zero length
 *                                   lies in device memory and is NOT detected: it is such a breach.  Waits for the stream.
 *   ss_count_leftmost_set_device    *count = the number of selected occurrences.  Waits for the stream.
 *   ss_find_all_leftmost_set_device *count = that number; d_offsets[0 .. min(count, capacity)) = the leftmost selected offsets,
 *                                   ascending, and d_ranks the ranks of the selected needles (ss_needle_set_ranks).  Either array
 *                                   may be NULL; capacity == 0: count only.  Waits for the stream.
 *   ss_replace_set_device           replacements[k] (host memory, replacement_lens[k] bytes, may be 0) belongs to needle k as given
 *                                   to ss_needle_set_new; `needles` must equal the set's `needles` stat.  Needles that share a rank
 *                                   must carry equal replacements.  *count is the number of selections and *out_len = len + the sum
 *                                   over the selections of (replacement length - needle length), computed with overflow checks:
 *                                   count * (the longest replacement) + len must fit 64 bits.  If out_capacity < *out_len, nothing
 *                                   is written and the call returns SS_OK: the caller sizes the buffer and calls again.  Otherwise
 *                                   d_out[0, *out_len) is the substituted view and nothing is written at *out_len or beyond.  d_out
 *                                   may have any alignment and must not intersect the haystack.  Waits for the stream.
 *   ss_needle_set_lengths           lengths[r] = the length of the needle of rank r (`distinct` entries, host memory), so that a
 *                                   caller of the primitive can turn ranks into lengths.
 * Refused with SS_ERR_ARGUMENT and a message that says why, nothing written: NULL result pointers and a NULL set; SS_BOUND_LINE,
 * SS_CONTEXT_INVERT and unknown bits in `how`; a mismatch of SS_BOUND_NOCASE with the set's fold; a set that holds the empty needle
 * (the haystack calls); a set made on another device than the current one; a capturing stream; d_selected == d_offsets, a NULL
 * d_offsets or d_lengths with count > 0 and count >= 2^48 in the primitive; `needles` other than the set's, a NULL replacement with a
 * length, unequal replacements of one rank, a d_out range that intersects the haystack's range, a NULL d_out where the output fits
 * the capacity and holds a byte, and an overflow of *out_len in ss_replace_set_device.  A failed temporary allocation returns
 * SS_ERR_NOMEM or SS_ERR_HIP with nothing written, and temporary memory is returned on every way out.
 *
 * Cost: the haystack calls run ss_count_set_device for the total T of pairs (T == 0 ends the call), ss_find_all_set_device into
 * temporary device memory of 12 bytes per pair (the precedent of ss_find_all_disjoint_device), and the primitive on those pairs;
 * the lengths come on the device from a per-rank table uploaded once per call, so no list of lengths is stored.  The primitive's
 * records are another 8 bytes per entry: 20 bytes per pair in all, returned inside the call (the 4,585-word list on 1 GiB of text:
 * 898 million pairs, 10.8 GB of pairs and 7.2 GB of records).  The selection works on blocks of SS_LEFTMOST_BLOCK entries staged in
 * LDS: an entry that is no candidate (the next offset is equal) hands on to its neighbour, a candidate to the first entry at or
 * beyond its end; pointer doubling gives every entry the selections of the walk that starts at it and the terminal it ends on; a
 * one-workgroup chain pass runs over the blocks, re-synchronising at every head (an entry that stands the list's largest length or
 * more beyond its predecessor), then a prefix, then an emit pass over the blocks that hold one of the first `capacity` selections.
 * ss_replace_set_device adds the output start of every selection (a block scan in LDS over the prefix kernel) and a copy pass
 * whose grid runs over the OUTPUT, one workgroup per SS_OUTPUT_CHUNK bytes cut from the 16-byte aligned address at or below d_out:
 * a 16-byte unit that lies inside one replacement or one gap of haystack text is one 16-byte load and ONE 16-byte store, a unit
 * that holds a border is composed in registers and stored once, only the units cut by d_out's own first and last byte are stored
 * byte by byte.  Every output byte is stored exactly once, no load touches a 16-byte block that holds no byte of the view or of
 * the (padded) replacement blob, no workgroup waits for another, there is no global atomic and the output depends on the input
 * alone.  Design and measurements: DESIGN.md 5.18.
 *
 * Out of scope: a scan that emits only the longest pair per offset; a host-side proof that a set cannot overlap itself (which
 * would let the call be its model); SS_BOUND_LINE and inverted forms; async / capturable, batched, plan, sharded, service and
 * host / file forms; regular expressions and back-references in the replacements.
 */
#ifndef SLICESLICE_HIP_LEFTMOST_H
#define SLICESLICE_HIP_LEFTMOST_H

#include "sliceslice_hip_output.h"

#define SS_LEFTMOST_BLOCK 4096u     /* entries per workgroup of the selection kernels */

#ifdef __cplusplus
extern "C" {
#endif

SS_API int ss_select_leftmost_device(const ss_needle_set *set, const uint64_t *d_offsets, const uint64_t *d_lengths, uint64_t count,
                                     void *hip_stream, uint64_t *d_selected, uint64_t *d_which, uint64_t capacity, uint64_t *selected);
SS_API int ss_count_leftmost_set_device(const ss_needle_set *set, const void *d_haystack, size_t len, unsigned how, void *hip_stream,
                                        uint64_t *count);
SS_API int ss_find_all_leftmost_set_device(const ss_needle_set *set, const void *d_haystack, size_t len, unsigned how, void *hip_stream,
                                           uint64_t *d_offsets, uint32_t *d_ranks, uint64_t capacity, uint64_t *count);
SS_API int ss_replace_set_device(const ss_needle_set *set, const void *d_haystack, size_t len, unsigned how,
                                 const void *const *replacements, const size_t *replacement_lens, uint32_t needles, void *hip_stream,
                                 void *d_out, uint64_t out_capacity, uint64_t *out_len, uint64_t *count);
SS_API int ss_needle_set_lengths(const ss_needle_set *set, uint64_t *lengths);

#ifdef __cplusplus
}
#endif
#endif /* SLICESLICE_HIP_LEFTMOST_H */
