/* sliceslice_hip_anyof.h - the lines that match ANY OF SEVERAL NEEDLES (grep -e A -e B, grep -f FILE; with -c, -n, -i, -w, -x, -v and
 * -A / -B / -C), and the ordered union of ascending lists of line numbers.  An OPT-IN component shipped in a library of its own.
 *
 *   libsliceslice_hip_anyof.so    the context library's objects PLUS the union kernels (sliceslice-rs_amd/csrc/ss_anyof.hip): every
 *                                 function of sliceslice_hip.h, sliceslice_hip_matches.h, sliceslice_hip_lines.h,
 *                                 sliceslice_hip_nocase.h, sliceslice_hip_bounded.h, sliceslice_hip_inverted.h and
 *                                 sliceslice_hip_context.h and the three below.  Linked INSTEAD of libsliceslice_hip.so; searchers
 *                                 belong to the library that made them.
 *
 * Rule:      Lines, the delimiter, line numbers, the record (begin, end, number) and `kind` are sliceslice_hip_lines.h's and
 *            sliceslice_hip_context.h's, word for word.  `how` takes the bits of ss_find_lines_context_device (SS_BOUND_NOCASE,
 *            SS_BOUND_WORD, SS_BOUND_LINE, SS_CONTEXT_INVERT) and applies to every needle.  S_k is the set of lines that the
 *            NON-inverted model call for how & ~SS_CONTEXT_INVERT selects for needle k, U the union of the S_k, N the number of
 *            lines.  The selected set S is U, or {1 .. N} \ U with SS_CONTEXT_INVERT.
 *   ss_count_lines_anyof_device   *lines = |S|.
 *   ss_find_lines_anyof_device    what ss_lines_around_device returns for S with `before` / `after`; *selected = |S|.
 *   The order of the needles, a needle given twice and a needle that is a prefix of another never change the result.  The empty
 *   needle selects every line, unless the model refuses it (SS_BOUND_WORD / SS_BOUND_LINE).  needles == 1 gives byte for byte
 *   what the model call and ss_find_lines_context_device give.  GNU grep selects the same lines (tests/golden/anyof_kat.json).
 *
 *   ss_union_numbers_device       the primitive.  `s` names the device and its scratch only; its needle is never looked at.
 *                                 `offsets` is a HOST array of lists + 1 ascending indices into d_numbers (CSR form, as in
 *                                 ss_find_all_batched): list k is d_numbers[offsets[k], offsets[k + 1]), in device memory; a list
 *                                 may be empty.  Every list must be STRICTLY ASCENDING - the caller's contract, as in
 *                                 ss_lines_around_device.  A 0 and a number above `limit` select nothing.  The output is each
 *                                 value of the union once, ascending; with complement != 0 it is every number of 1 .. limit that
 *                                 is in no list.  *total = the size of the output; the leftmost min(total, capacity) values are
 *                                 written, nothing at index capacity or beyond.  capacity == 0 or d_out == NULL: count only.
 *                                 lists == 0 gives the empty union (with complement: 1 .. limit).  limit == 0: 0 with no launch.
 *                                 On a breach of the contract (a list that repeats or descends) nothing faults and nothing is
 *                                 written outside the first min(total, capacity) slots, and every written value lies in
 *                                 1 .. limit; beyond that the output is unspecified.
 *                                 Refused with SS_ERR_ARGUMENT: lists > SS_ANYOF_MAX_NEEDLES, descending offsets, a limit that
 *                                 needs more than 2^31 - 1 segments of SS_ANYOF_SEGMENT_LINES numbers, a capturing stream.
 *   The two line calls work like ss_find_lines_context_device, through public entry points only: per needle the model's count,
 *   then the model's record call with d_number only into ONE temporary device buffer of 8 bytes per selected line summed over
 *   the needles (host-side CSR offsets); N, which SS_CONTEXT_INVERT needs and which serves as `limit`, from the delimiter census
 *   (ss_lines_around_device for the single number 1 with before = 0, after = 2^64 - 1 and capacity 0), never from the empty
 *   needle's byte-wise pass; then the union, and for the find call ss_lines_around_device on its result.  Refusals and messages
 *   of the models pass through with nothing written (a case-sensitive searcher under SS_BOUND_NOCASE, the empty needle under
 *   SS_BOUND_WORD / SS_BOUND_LINE); unknown bits in `how` are refused here.  Refused here with SS_ERR_ARGUMENT as well:
 *   needles == 0, needles > SS_ANYOF_MAX_NEEDLES, a NULL entry in `searchers`, searchers of different devices (a searcher of this
 *   library carries no device: every needle is searched on the CURRENT device, the one that holds the haystack, so the case cannot
 *   arise through this header).  The temporary memory is returned on every way out; a failed allocation returns SS_ERR_NOMEM or
 *   SS_ERR_HIP with nothing written.  All three calls wait for the stream; none is capturable (a capturing stream is refused
 *   with SS_ERR_ARGUMENT) and there is no async form.
 *
 * Cost: K needles cost K times the model's passes - one count and at most two record passes each - plus ONE census pass and the
 * union (with context or records: the primitive of sliceslice_hip_context.h, which holds a second census pass).  The union reads
 * the numbers twice (count, emit) and never touches the haystack: one workgroup per segment of SS_ANYOF_SEGMENT_LINES numbers,
 * an 8 KiB bitmap in LDS, one 8-byte count per segment, their prefix, an emit pass that skips the segments at or above the
 * capacity.  Scratch is 16 bytes per segment plus the lists' offsets, never per line; there is no global atomic and the output is
 * deterministic.  Rates measured on an MI355X are in DESIGN.md 5.13.
 *
 * Out of scope: ONE scan that filters for all needles in a single pass over the haystack (the follow-up that this header makes
 * measurable: sliceslice_hip_needleset.h compiles the needles into a set and selects the same lines in one scan); async and capturable forms; batched, plan, sharded, service and host / file forms; -m; -o with several needles; a
 * `how` per needle; regular expressions; multi-byte terminators; the text of the lines (sliceslice_hip_output.h gathers and
 * numbers the records of any line call on the device).
 */
#ifndef SLICESLICE_HIP_ANYOF_H
#define SLICESLICE_HIP_ANYOF_H

#include "sliceslice_hip_context.h"

#define SS_ANYOF_MAX_NEEDLES   65536u   /* needles (or lists) per call */
#define SS_ANYOF_SEGMENT_LINES 65536u   /* line numbers per workgroup of the union kernels */

#ifdef __cplusplus
extern "C" {
#endif

SS_API int ss_union_numbers_device(const ss_searcher *s, const uint64_t *d_numbers, const uint64_t *offsets, uint32_t lists,
                                   uint64_t limit, int complement, void *hip_stream, uint64_t *d_out, uint64_t capacity,
                                   uint64_t *total);
SS_API int ss_count_lines_anyof_device(const ss_searcher *const *searchers, uint32_t needles, const void *d_haystack, size_t len,
                                       int delimiter, unsigned how, void *hip_stream, uint64_t *lines);
SS_API int ss_find_lines_anyof_device(const ss_searcher *const *searchers, uint32_t needles, const void *d_haystack, size_t len,
                                      int delimiter, unsigned how, uint64_t before, uint64_t after, void *hip_stream,
                                      uint64_t *d_begin, uint64_t *d_end, uint64_t *d_number, uint8_t *d_kind, uint64_t capacity,
                                      uint64_t *lines, uint64_t *selected);

#ifdef __cplusplus
}
#endif
#endif /* SLICESLICE_HIP_ANYOF_H */
