/* sliceslice_hip_nocase.h - every occurrence of a needle, and the lines that contain it, IGNORING ASCII CASE (grep -i with -o -b,
 * -c, -n).  An OPT-IN component shipped in a library of its own, like the scans it is built on.
 *
 *   libsliceslice_hip_nocase.so  the lines library's objects PLUS the case-folding scans (sliceslice-rs_amd/csrc/ss_nocase.hip,
 *                                scan_inst_nocase.hip): every function of sliceslice_hip.h, sliceslice_hip_matches.h and
 *                                sliceslice_hip_lines.h and the seven below.  Linked INSTEAD of libsliceslice_hip.so; searchers belong
 *                                to the library that made them.
 *
 * Rule:      two bytes are equal ignoring case when they are equal, or when both are letters 'A'..'Z' / 'a'..'z' (0x41-0x5A,
 *            0x61-0x7A) that differ only in bit 5.  Every other byte compares exactly: '@' '[' '`' '{' next to the letter ranges,
 *            and every byte >= 0x80 - 0xC1-0xDA and 0xE1-0xFA included, whose low seven bits look like letters.  This is grep -i
 *            in the C locale, Rust's eq_ignore_ascii_case, Python's hay.lower() / needle.lower() on bytes.
 * The fold happens inside the scan kernels, on the bytes as they are compared: the haystack is read once by the count calls and at
 * most twice by the record calls, as in the case-sensitive forms, and no folded copy of it is made.
 * Everything else is sliceslice_hip_matches.h's and sliceslice_hip_lines.h's, word for word: overlapping occurrences, the empty
 * needle, n > len, 64-bit ascending offsets and records, nothing written at index `capacity` or beyond, no byte outside a
 * misaligned view counts, no dependence on position, ss_searcher_set_filter3 or launch tuning, the census neither started nor read.
 * THE DELIMITER IS NEVER FOLDED: delimiter 'A' cuts at 'A' only, not at 'a'.  A searcher whose (folded) needle holds the delimiter
 * byte itself matches no line, as in ss_count_lines_device; one that holds only its other case can match (needle "a", delimiter 'A').
 *
 *   ss_searcher_new_nocase              folds a copy of the needle to lower case, then does exactly what ss_searcher_new does.  The
 *                                       result is an ordinary searcher whose needle is the folded copy: every case-sensitive
 *                                       call works on it (the folded needle against unfolded haystack bytes).
 *   ss_count_nocase_device, ss_count_nocase_device_async, ss_find_all_nocase_device
 *                                       the argument lists, waits and capture rules of ss_count_device, ss_count_device_async
 *                                       (capturable into a hipGraph) and ss_find_all_device.
 *   ss_count_lines_nocase_device, ss_count_lines_nocase_device_async, ss_find_lines_nocase_device
 *                                       those of ss_count_lines_device, ss_count_lines_device_async (refuses a capturing stream)
 *                                       and ss_find_lines_device.
 * The six scan calls accept ANY searcher whose needle holds no byte in 'A'..'Z', from whatever constructor (with_position,
 * set_filter3 and the census state included), and return SS_ERR_ARGUMENT with a message that names ss_searcher_new_nocase otherwise.
 *
 * Out of scope: early-exit search / find ignoring case (they would need twins of the 22 scan kernels;
 * ss_find_all_nocase_device with capacity 1 answers the question without the early exit); batched, plan, sharded, service and
 * host / file forms; Unicode or locale folding; folding the delimiter.  Rates measured on an MI355X are in DESIGN.md 5.9.
 */
#ifndef SLICESLICE_HIP_NOCASE_H
#define SLICESLICE_HIP_NOCASE_H

#include "sliceslice_hip_lines.h"

#ifdef __cplusplus
extern "C" {
#endif

SS_API int ss_searcher_new_nocase(const uint8_t *needle, size_t n, ss_searcher **out);
SS_API int ss_count_nocase_device(const ss_searcher *s, const void *d_haystack, size_t len, void *hip_stream, uint64_t *count);
SS_API int ss_count_nocase_device_async(const ss_searcher *s, const void *d_haystack, size_t len, void *hip_stream, uint64_t *d_count);
SS_API int ss_find_all_nocase_device(const ss_searcher *s, const void *d_haystack, size_t len, void *hip_stream, uint64_t *d_offsets,
                                     uint64_t capacity, uint64_t *count);
SS_API int ss_count_lines_nocase_device(const ss_searcher *s, const void *d_haystack, size_t len, int delimiter, void *hip_stream,
                                        uint64_t *lines);
SS_API int ss_count_lines_nocase_device_async(const ss_searcher *s, const void *d_haystack, size_t len, int delimiter, void *hip_stream,
                                              uint64_t *d_lines);
SS_API int ss_find_lines_nocase_device(const ss_searcher *s, const void *d_haystack, size_t len, int delimiter, void *hip_stream,
                                       uint64_t *d_begin, uint64_t *d_end, uint64_t *d_number, uint64_t capacity, uint64_t *lines);

#ifdef __cplusplus
}
#endif
#endif /* SLICESLICE_HIP_NOCASE_H */
