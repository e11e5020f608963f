/* sliceslice_hip_context.h - matching lines WITH THEIR CONTEXT LINES (grep -A / -B / -C with -n; it combines with -i, -w, -x and
 * -v), and the records of any set of line numbers.  An OPT-IN component shipped in a library of its own, like the scans it stands on.
 *
 *   libsliceslice_hip_context.so  the inverted library's objects PLUS the context kernels (sliceslice-rs_amd/csrc/ss_context.hip):
 *                                 every function of sliceslice_hip.h, sliceslice_hip_matches.h, sliceslice_hip_lines.h,
 *                                 sliceslice_hip_nocase.h, sliceslice_hip_bounded.h and sliceslice_hip_inverted.h and the two below.
 *                                 Linked INSTEAD of libsliceslice_hip.so; searchers belong to the library that made them.
 *
 * Rule:      Lines, the delimiter, line numbers and the record (begin, end, number) are sliceslice_hip_lines.h's, word for word.
 *            S is the ascending set of line numbers that a model call selects, N the number of lines (the empty needle's
 *            ss_count_lines_device).  With `before` = b and `after` = a the output is every line whose number lies in the union
 *            over s in S of [max(1, s - b), min(N, s + a)], each line once, in ascending order.
 *   kind     1 for a line of S (grep prints `number:`), 0 for a context line (grep prints `number-`).
 *   --       grep's separator stands wherever two consecutive output numbers differ by more than 1; the library returns no
 *            separators, the caller derives them (sliceslice_hip_output.h writes them, with the lines' text, on the device).
 *   before, after   any uint64_t value: the additions and subtractions saturate, 2^64 - 1 means "to the ends of the view".
 *   An empty S gives an empty output whatever b and a are.
 * Bytes outside the view never count: neither a delimiter just in front of a misaligned view nor one just behind its end.
 * Everything is 64-bit (haystacks above 4 GiB included).
 *
 *   ss_lines_around_device        the primitive.  `s` names the device and its scratch only; its needle is never looked at.
 *                                 d_numbers[0, count) are 1-based line numbers in device memory, STRICTLY ASCENDING - the caller's
 *                                 contract.  A 0 and a number above N select nothing and give no context.  *lines = the size of
 *                                 the output; the leftmost min(total, capacity) entries of each non-NULL array are written, nothing
 *                                 at index capacity or beyond.  capacity == 0 or all four arrays NULL: count only.  count == 0 or
 *                                 len == 0: 0 with no launch.  With before = after = 0 it returns the records of the listed lines,
 *                                 all of kind 1 - the way to get records, or context, for lines found by other means (the union of
 *                                 several needles' numbers, sed -n 'Np').
 *                                 On a breach of the contract (numbers that repeat or descend) nothing faults and nothing is
 *                                 written outside the first min(total, capacity) entries, but the output is unspecified: every
 *                                 entry still owns a range inside 1 .. N that holds it, cut only by neighbours that ARE in order,
 *                                 so lines may repeat, the order may break, and records of lines that the searches among the
 *                                 numbers miss stay unwritten.
 *   ss_find_lines_context_device  three steps: the model's count for `how` (*selected), the model's record call with d_number only
 *                                 into temporary device memory of 8 bytes per selected line, and the primitive.  The model by `how`:
 *       0                                          ss_find_lines_device
 *       SS_BOUND_NOCASE alone                      ss_find_lines_nocase_device
 *       with SS_BOUND_WORD or SS_BOUND_LINE        ss_find_lines_bounded_device
 *       with SS_CONTEXT_INVERT                     ss_find_lines_inverted_device, with the remaining bits
 *                                 Refusals and their messages are the models' own, passed through with nothing written; unknown
 *                                 bits in `how` are refused here.  A failed temporary allocation returns SS_ERR_NOMEM or SS_ERR_HIP
 *                                 with nothing written; the memory is returned inside the call.
 * Argument checks, error codes and ss_last_error follow ss_find_lines_device.  Both functions wait for the stream; neither is
 * capturable (a capturing stream is refused with SS_ERR_ARGUMENT) and there is no async form.
 *
 * Cost: the primitive reads the haystack ONCE (the delimiter census: one workgroup per part of SS_CONTEXT_PART_BYTES, cut at
 * multiples of that size from the 16-byte aligned address at or below the view, 16-byte non-temporal loads, one 8-byte store per
 * part), plus a second time only in the parts that hold an end or a beginning of an output line below the capacity.  The context
 * call adds its model's passes.  Scratch is 16 bytes per part plus 8 bytes and a little per INPUT number, never per line of the
 * haystack; there is no global atomic.  Rates measured on an MI355X are in DESIGN.md 5.12.
 *
 * Out of scope: -m; async and capturable forms; batched, plan, sharded, service and host / file forms; a form that never
 * materialises the selected numbers; several needles at once (-e A -e B, -f FILE: sliceslice_hip_anyof.h unites the numbers of
 * several needles' lines on the device and hands them to the primitive above, sliceslice_hip_needleset.h finds them in one scan); multi-byte terminators; regular expressions.
 */
#ifndef SLICESLICE_HIP_CONTEXT_H
#define SLICESLICE_HIP_CONTEXT_H

#include "sliceslice_hip_inverted.h"

#define SS_CONTEXT_INVERT 8u            /* with the SS_BOUND_* bits in `how`: the model is the inverted call */
#define SS_CONTEXT_PART_BYTES 65536u    /* bytes of the view per workgroup of the census and the select pass */

#ifdef __cplusplus
extern "C" {
#endif

SS_API int ss_lines_around_device(const ss_searcher *s, const void *d_haystack, size_t len, int delimiter, const uint64_t *d_numbers,
                                  uint64_t count, uint64_t before, uint64_t after, void *hip_stream, uint64_t *d_begin,
                                  uint64_t *d_end, uint64_t *d_number, uint8_t *d_kind, uint64_t capacity, uint64_t *lines);
SS_API int ss_find_lines_context_device(const ss_searcher *s, const void *d_haystack, size_t len, int delimiter, unsigned how,
                                        uint64_t before, uint64_t after, void *hip_stream, uint64_t *d_begin, uint64_t *d_end,
                                        uint64_t *d_number, uint8_t *d_kind, uint64_t capacity, uint64_t *lines, uint64_t *selected);

#ifdef __cplusplus
}
#endif
#endif /* SLICESLICE_HIP_CONTEXT_H */
