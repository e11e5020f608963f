/* sliceslice_hip_inverted.h - the lines that do NOT match: their number and their records (grep -v with -c and -n; it combines with
 * -i, -w and -x).  An OPT-IN component shipped in a library of its own, like the scans it is built on.
 *
 *   libsliceslice_hip_inverted.so  the bounded library's objects PLUS the inverted kernels (sliceslice-rs_amd/csrc/ss_inverted.hip,
 *                                  scan_inst_inverted.hip, scan_inst_inverted_nocase.hip): every function of sliceslice_hip.h,
 *                                  sliceslice_hip_matches.h, sliceslice_hip_lines.h, sliceslice_hip_nocase.h and
 *                                  sliceslice_hip_bounded.h and the three below.  Linked INSTEAD of libsliceslice_hip.so;
 *                                  searchers belong to the library that made them.
 *
 * Rule:      `how` names the NON-INVERTED call whose complement is taken, with the bits of sliceslice_hip_bounded.h and no new ones:
 *   0                                  ss_count_lines_device / ss_find_lines_device                        (grep -v)
 *   SS_BOUND_NOCASE                    ss_count_lines_nocase_device / ss_find_lines_nocase_device          (grep -v -i)
 *   SS_BOUND_WORD [| SS_BOUND_NOCASE]  the bounded line calls with the same `how`                           (grep -v -w [-i])
 *   SS_BOUND_LINE [| SS_BOUND_NOCASE]  the bounded line calls with the same `how`                           (grep -v -x [-i])
 *            A line is selected when it does NOT match in that call.  For every input, inverted count + non-inverted count = the
 *            number of lines (what the empty needle's ss_count_lines_device returns); the two record sets are disjoint and their
 *            merge is the empty needle's record set.
 * Lines, the delimiter, the records (begin, end, number), their 64-bit ascending order, the capacity rule and NULL arrays are
 * sliceslice_hip_lines.h's, word for word: nothing is written at index `capacity` or beyond, each of d_begin / d_end / d_number may
 * be NULL.  So are the independence from position, ss_searcher_set_filter3 and launch tuning, and the census is neither started
 * nor read.
 *   - An unterminated last line is a line; it is selected when it holds no kept occurrence.
 *   - An empty haystack has no line: 0.
 *   - A needle longer than the view, or one that holds the delimiter, matches no line: EVERY line is selected (the models return 0
 *     there; this call returns the number of lines).
 *   - The empty needle with `how` = 0 or SS_BOUND_NOCASE matches every line: 0, nothing written.
 *   - The empty needle with SS_BOUND_WORD or SS_BOUND_LINE is refused, as in the bounded calls (GNU grep's -v -x '' selects the
 *     non-empty lines; that stays out of scope).
 * There is no inverted OCCURRENCE form: occurrences have no complement.
 *
 *   ss_count_lines_inverted_device, ss_count_lines_inverted_device_async, ss_find_lines_inverted_device
 *                                       the argument lists, waits and capture rules of ss_count_lines_device,
 *                                       ss_count_lines_device_async (refuses a capturing stream) and ss_find_lines_device, with
 *                                       `how` behind the delimiter, exactly as in the bounded line calls.
 * Refused with SS_ERR_ARGUMENT and a message that says why, nothing written: unknown bits in `how`; SS_BOUND_WORD and SS_BOUND_LINE
 * together; an upper-case needle byte with SS_BOUND_NOCASE (the nocase calls' check, with their message); a delimiter outside
 * 0 .. 255; the empty needle with a bound.
 *
 * Cost: the count runs its model's launches and one single-thread kernel more - the haystack is read once.  The record call reads
 * the haystack a second time wherever a part closes a selected line below the capacity, which for most needles is nearly
 * everywhere.  Rates measured on an MI355X are in DESIGN.md 5.11.
 *
 * Out of scope: batched, plan, sharded, service and host / file forms; context lines (-A / -B / -C: they are
 * sliceslice_hip_context.h's, which takes these calls as models); several needles at once (-e A -e B, -f FILE: they are
 * sliceslice_hip_anyof.h's, whose SS_CONTEXT_INVERT selects the lines that match none of them, and in one scan for a whole set
 * sliceslice_hip_needleset.h's); -m; the empty needle with -w / -x;
 * multi-byte terminators; regular expressions.
 */
#ifndef SLICESLICE_HIP_INVERTED_H
#define SLICESLICE_HIP_INVERTED_H

#include "sliceslice_hip_bounded.h"

#ifdef __cplusplus
extern "C" {
#endif

SS_API int ss_count_lines_inverted_device(const ss_searcher *s, const void *d_haystack, size_t len, int delimiter, unsigned how,
                                          void *hip_stream, uint64_t *lines);
SS_API int ss_count_lines_inverted_device_async(const ss_searcher *s, const void *d_haystack, size_t len, int delimiter, unsigned how,
                                                void *hip_stream, uint64_t *d_lines);
SS_API int ss_find_lines_inverted_device(const ss_searcher *s, const void *d_haystack, size_t len, int delimiter, unsigned how,
                                         void *hip_stream, uint64_t *d_begin, uint64_t *d_end, uint64_t *d_number, uint64_t capacity,
                                         uint64_t *lines);

#ifdef __cplusplus
}
#endif
#endif /* SLICESLICE_HIP_INVERTED_H */
