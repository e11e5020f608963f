/* sliceslice_hip_bounded.h - every occurrence of a needle, and the lines that contain it, kept only where the needle stands as a
 * WHOLE WORD or is the WHOLE LINE (grep -w, grep -x with -o -b, -c, -n; both combine with -i).  An OPT-IN component shipped in a
 * library of its own, like the scans it is built on.
 *
 *   libsliceslice_hip_bounded.so  the nocase library's objects PLUS the bounded scans (sliceslice-rs_amd/csrc/ss_bounded.hip,
 *                                 scan_inst_bounded.hip, scan_inst_bounded_nocase.hip): every function of sliceslice_hip.h,
 *                                 sliceslice_hip_matches.h, sliceslice_hip_lines.h and sliceslice_hip_nocase.h and the six below.
 *                                 Linked INSTEAD of libsliceslice_hip.so; searchers belong to the library that made them.
 *
 * Rule:      the word bytes W are '0'..'9', 'A'..'Z', 'a'..'z' and '_' (the C locale); no byte >= 0x80 is a word byte.
 *            An occurrence of a needle of n >= 1 bytes at offset p of the view [0, len) has a LEFT neighbour hay[p - 1], absent when
 *            p == 0, and a RIGHT neighbour hay[p + n], absent when p + n == len.  A byte outside the view is absent, whatever
 *            memory holds there (a misaligned view inside a larger buffer).  With `how` =
 *   SS_BOUND_WORD   in the occurrence forms (count, find_all): each neighbour is absent or not in W.
 *                   in the line forms (count_lines, find_lines; delimiter d): each neighbour is absent, equal to d, or not in W - a
 *                   delimiter that is itself a word byte still ends a word (grep's "at the beginning / end of the line").
 *   SS_BOUND_LINE   line forms only: each neighbour is absent or equal to d.  The number of matching lines is the number of lines
 *                   equal to the needle.
 *   | SS_BOUND_NOCASE   either of the two, with bytes compared as in sliceslice_hip_nocase.h.  The neighbour classes do not
 *                   change (W is closed under the fold) and the delimiter is never folded.  The searcher's needle must hold no
 *                   'A'..'Z': the nocase calls' check, with their message.
 * The test looks at the two neighbours only, never at the needle's own bytes: the needle ".foo" does not occur as a word in
 * "a.foo" (GNU grep -w agrees).  Occurrences overlap, as in sliceslice_hip_matches.h, and a line matches when at least one of its
 * occurrences qualifies - also when others in front of it do not.
 * Everything else is sliceslice_hip_matches.h's and sliceslice_hip_lines.h's, word for word: n > len gives 0, a needle that holds
 * the delimiter matches no line, 64-bit ascending offsets and records, nothing written at index `capacity` or beyond, each of
 * d_begin / d_end / d_number may be NULL, no dependence on position, ss_searcher_set_filter3 or launch tuning, the census neither
 * started nor read.  The test runs inside the scan kernels on the occurrences they confirm: the haystack is read once by the count
 * calls and at most twice by the record calls, and no list of unfiltered offsets is made.
 *
 *   ss_count_bounded_device, ss_count_bounded_device_async, ss_find_all_bounded_device
 *                                       the argument lists, waits and capture rules of ss_count_device, ss_count_device_async
 *                                       (capturable into a hipGraph) and ss_find_all_device, with `how` in front of the stream.
 *   ss_count_lines_bounded_device, ss_count_lines_bounded_device_async, ss_find_lines_bounded_device
 *                                       those of ss_count_lines_device, ss_count_lines_device_async (refuses a capturing stream)
 *                                       and ss_find_lines_device, with `how` behind the delimiter.
 * Refused with SS_ERR_ARGUMENT and a message that says why, nothing written: the empty needle; neither SS_BOUND_WORD nor
 * SS_BOUND_LINE (the message names the plain or the nocase call to use); both; SS_BOUND_LINE in an occurrence form; unknown bits.
 *
 * Out of scope: the empty needle (GNU grep's answers for -w '' are a special case of its own); batched, plan, sharded, service and
 * host / file forms; early-exit search / find with bounds; Unicode or locale word classes; a caller-supplied byte class;
 * context lines and -m here.  (-v is sliceslice_hip_inverted.h's; context lines around the lines of these calls are
 * sliceslice_hip_context.h's; the lines that match any of several needles are sliceslice_hip_anyof.h's, in one scan for a compiled set
 * sliceslice_hip_needleset.h's.)  Rates measured on an
 * MI355X are in DESIGN.md 5.10.
 */
#ifndef SLICESLICE_HIP_BOUNDED_H
#define SLICESLICE_HIP_BOUNDED_H

#include "sliceslice_hip_nocase.h"

#define SS_BOUND_WORD   1u
#define SS_BOUND_LINE   2u
#define SS_BOUND_NOCASE 4u

#ifdef __cplusplus
extern "C" {
#endif

SS_API int ss_count_bounded_device(const ss_searcher *s, const void *d_haystack, size_t len, unsigned how, void *hip_stream,
                                   uint64_t *count);
SS_API int ss_count_bounded_device_async(const ss_searcher *s, const void *d_haystack, size_t len, unsigned how, void *hip_stream,
                                         uint64_t *d_count);
SS_API int ss_find_all_bounded_device(const ss_searcher *s, const void *d_haystack, size_t len, unsigned how, void *hip_stream,
                                      uint64_t *d_offsets, uint64_t capacity, uint64_t *count);
SS_API int ss_count_lines_bounded_device(const ss_searcher *s, const void *d_haystack, size_t len, int delimiter, unsigned how,
                                         void *hip_stream, uint64_t *lines);
SS_API int ss_count_lines_bounded_device_async(const ss_searcher *s, const void *d_haystack, size_t len, int delimiter, unsigned how,
                                               void *hip_stream, uint64_t *d_lines);
SS_API int ss_find_lines_bounded_device(const ss_searcher *s, const void *d_haystack, size_t len, int delimiter, unsigned how,
                                        void *hip_stream, uint64_t *d_begin, uint64_t *d_end, uint64_t *d_number, uint64_t capacity,
                                        uint64_t *lines);

#ifdef __cplusplus
}
#endif
#endif /* SLICESLICE_HIP_BOUNDED_H */
