/* sliceslice_hip_lines.h - the LINES that contain a needle: how many (grep -c), and which (grep -n).  An OPT-IN component shipped
 * in a library of its own, like the all-matches scan it is built on.
 *
 *   libsliceslice_hip_lines.so  the matches library's objects PLUS the matching-lines scan (sliceslice-rs_amd/csrc/ss_lines.hip,
 *                               scan_inst_lines.hip): every function of sliceslice_hip.h, of sliceslice_hip_matches.h and the three
 *                               below.  Linked INSTEAD of libsliceslice_hip.so; searchers belong to the library that made them.
 *
 * Delimiter: ONE byte, any value 0 .. 255 ('\n' for text, 0 for grep -z); anything else is SS_ERR_ARGUMENT.
 * Lines:     the view [0, len) is cut at every delimiter byte; a delimiter belongs to no line; the bytes behind the last delimiter
 *            form a last line only if there are any (Python: data.split(delim) with a trailing empty piece dropped).  An empty
 *            haystack has no line; the empty lines between two delimiters are lines.
 * A line MATCHES when at least one occurrence of the needle lies wholly inside it.  Therefore
 *            a needle that contains the delimiter (needle == [delimiter] included) matches no line: the answer is 0, not an error;
 *            the empty needle matches every line, the empty ones included: the count is the number of lines;
 *            a line counts once, however many occurrences it holds.
 * A record per matching line, in ascending order, all three 64-bit (haystacks above 4 GiB included):
 *            begin   offset of the line's first byte
 *            end     offset of the delimiter that closes it, or len for a last line without one; end - begin is the line's length
 *            number  1-based: the number of delimiters in front of begin, plus one (what grep -n prints)
 * Bytes outside the view never count - neither delimiters nor needle copies in the aligned chunks the kernels load around a
 * misaligned view.  The result never depends on the searcher's position, on ss_searcher_set_filter3 or on launch tuning, and the
 * calls neither start nor read the census: ss_searcher_tuning_state is the same before and after them.
 *
 * Argument checks, error codes and ss_last_error follow ss_find_all_device.
 *
 *   ss_count_lines_device        *lines = number of matching lines; waits for the stream.
 *   ss_count_lines_device_async  the same, stream-ordered, no host wait: the count lands in *d_lines (device memory, overwritten, no
 *                                initialisation needed).  The call owns its scratch the way ss_count_batched does - it goes back
 *                                behind an event recorded on the stream - and therefore REFUSES a capturing stream with
 *                                SS_ERR_ARGUMENT, exactly as ss_count_batched does.
 *   ss_find_lines_device         *lines = total number of matching lines; the leftmost min(total, capacity) records are written to
 *                                d_begin / d_end / d_number (each may be NULL independently: that array is not wanted); nothing at
 *                                index capacity or beyond is touched.  capacity == 0: count only.  Waits for the stream.
 *
 * The haystack is read once by the count calls and at most twice by ss_find_lines_device (only the workgroups that close one of
 * the first `capacity` matching lines read their part again; a caller who counts first to size the arrays, as the Python
 * find_lines(capacity=None) does, adds the count's pass); scratch is a few dozen bytes per workgroup, whatever the number of
 * matches, lines or delimiters.  Rates measured on an MI355X are in DESIGN.md 5.8.
 */
#ifndef SLICESLICE_HIP_LINES_H
#define SLICESLICE_HIP_LINES_H

#include "sliceslice_hip_matches.h"

#ifdef __cplusplus
extern "C" {
#endif

SS_API int ss_count_lines_device(const ss_searcher *s, const void *d_haystack, size_t len, int delimiter, void *hip_stream,
                                 uint64_t *lines);
SS_API int ss_count_lines_device_async(const ss_searcher *s, const void *d_haystack, size_t len, int delimiter, void *hip_stream,
                                       uint64_t *d_lines);
SS_API int ss_find_lines_device(const ss_searcher *s, const void *d_haystack, size_t len, int delimiter, void *hip_stream,
                                uint64_t *d_begin, uint64_t *d_end, uint64_t *d_number, uint64_t capacity, uint64_t *lines);

#ifdef __cplusplus
}
#endif
#endif /* SLICESLICE_HIP_LINES_H */
