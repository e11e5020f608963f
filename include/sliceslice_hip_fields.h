/* sliceslice_hip_fields.h - FIELDS first .. last OF EVERY LINE, located on the device: `cut -d, -f3`, `cut -f2-4`,
 * `awk '{print $2}'`, "column 5 of this TSV".  The answer is a list of (begin, end, number) records that ss_gather_ranges_device
 * (sliceslice_hip_output.h) turns into text.  An OPT-IN component shipped in a library of its own.
 *
 *   libsliceslice_hip_fields.so  the rewrite library's objects PLUS the field scan (sliceslice-rs_amd/csrc/ss_fields.hip): every
 *                                function of sliceslice_hip_rewrite.h and of the headers it includes, and those below.  Linked
 *                                INSTEAD of libsliceslice_hip.so; handles belong to the library that made them.
 *
 * THE RULE (everything else refers to it):
 *   Line        lines, the delimiter (one byte, any value), the last line and the line numbers are sliceslice_hip_lines.h's.  The
 *               delimiter is never a separator, even where the set holds it.
 *   Separator   a non-empty class of byte values in the four-word layout of sliceslice_hip_classes.h: `,`, `\t`, `[ \t]`.
 *   SS_FIELDS_EACH   (cut, CSV without quoting) every separator byte ends a field: a line with s separators has s + 1 fields, fields
 *               may be empty, an empty line has one empty field.
 *   SS_FIELDS_MERGE  (awk's default) the fields of a line are its maximal runs of bytes that are neither separator nor delimiter:
 *               leading and trailing separators make no field, a line of separators only has 0 fields.
 *   Selection   (first, last), both 64-bit: 1 <= first; last == 0 means "to the line's end", otherwise first <= last.  A line with
 *               n fields is selected when n >= first.
 *   Record      of a selected line: [begin, end) and the line's number.  begin is the first byte of field `first`.  If last != 0
 *               and n >= last, end is the end of field `last`; otherwise end is the line's end: the position of its delimiter, or
 *               the view's end.  In MERGE mode that means TRAILING SEPARATORS ARE KEPT when the line runs out of fields
 *               (`a b  ` with 2-5 gives `b  `).
 *   SS_FIELDS_KEEP_SHORT   lines that are not selected get an empty record, begin == end == the line's end.  The call then returns
 *               exactly one record per line and record k is line k + 1: a column aligned with its rows.
 *   Bytes outside [0, len) are absent, whatever memory holds there, and no load touches a 16-byte block that holds no byte of the
 *   view.  Offsets, counts and numbers are 64-bit.  Records ascend.
 *
 * THE LANGUAGE of ss_fields_parse is cut's single range: `K` is (K, K), `K-` is (K, 0), `K-M` is (K, M), `-M` is (1, M); K and M
 * are decimal, at least 1 and below 2^64.  Refused, naming the column (from 1) as ss_runs_parse does: an empty text, anything
 * else than digits and one `-`, 0, M < K, a number that does not fit 64 bits, and a comma list (`1,3`): make one call per range.
 *
 * Argument conventions are sliceslice_hip_runs.h's.
 *   ss_fields_new            the set (host memory, 4 words), the mode, (first, last) and flags -> a handle on the current device.
 *   ss_fields_free           NULL is allowed.
 *   ss_fields_info           mode, first, last, flags, the number of members and whether the set accepts `delimiter` (0 .. 255; a
 *                            negative one asks for nothing).
 *   ss_fields_parse          HOST ONLY: the language above -> (first, last).
 *   ss_count_fields_device   *lines_selected = the lines with n >= first (KEEP_SHORT changes nothing here), *lines_total = all
 *                            lines.  Waits for the stream.  THERE IS NO _async FORM: a field's number is carried from workgroup to
 *                            workgroup, which takes a summary per workgroup, temporary memory that grows with the view; a call
 *                            that takes it from the library's pool cannot be captured into a hipGraph.
 *   ss_find_fields_device    the first `capacity` records, ascending: d_begin[k], d_end[k], d_number[k] (any array may be NULL);
 *                            *total is always the full record count.  Capacity and NULL rules are ss_find_all_runs_device's: all
 *                            arrays NULL with a non-zero capacity is refused, capacity 0 is the sizing call.  Waits for the stream.
 * Refused with SS_ERR_ARGUMENT and a message, nothing written: NULL handles or result pointers; an unknown mode or flag;
 * first == 0; last non-zero and below first; an empty set; a set that is only the delimiter (in the scan calls); a NULL haystack
 * with len > 0; a handle made on another device; a capturing stream; all three arrays NULL with a non-zero capacity; a delimiter
 * that is no byte.
 *
 * Cost (fields_kernels.hpp, on the run kernels' geometry: 16 B per lane, 1 KiB per piece, 4 KiB per wave, 16 KiB per tile,
 * 128 KiB per workgroup).  A byte's field number is one plus the EVENTS since the last delimiter - EACH: separator bytes; MERGE:
 * bytes that begin a field.  The count is carried in the lane by a popcount restarted at its last delimiter, across the lanes of
 * a piece by one prefix sum and a ballot, across waves and tiles through LDS.  PASS 1 leaves 32 bytes per workgroup: its
 * delimiters, the events in front of its first and behind its last delimiter, and the record begins and ends of the lines that
 * begin inside it.  ONE workgroup then walks these summaries in order, SS_FIELDS_CARRY_CHUNK at a time - a workgroup with a
 * delimiter replaces the carry by its tail, one without adds its events - and leaves every workgroup's carry-in, line base and
 * ranks; it never reads the haystack.  The count ends there: the view is read once.  PASS 2 (find) runs the same grid over the
 * workgroups that hold one of the first `capacity` begins or ends.  No waiting between workgroups, no atomic; temporary device
 * memory is 80 bytes per workgroup; the output depends on the input alone.
 *
 * Out of scope: comma lists of ranges in one call; quoted CSV fields; multi-byte separators; a replace form; batched forms; an
 * output delimiter other than the gather call's terminator; an async / capturable count.
 */
#ifndef SLICESLICE_HIP_FIELDS_H
#define SLICESLICE_HIP_FIELDS_H

#include "sliceslice_hip_rewrite.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SS_FIELDS_EACH 0
#define SS_FIELDS_MERGE 1
#define SS_FIELDS_KEEP_SHORT 1u
#define SS_FIELDS_CARRY_CHUNK 256       /* workgroup summaries per step of the carry kernel */

typedef struct ss_fields ss_fields;

typedef struct ss_fields_stats {
    uint64_t mode;                          /* SS_FIELDS_EACH or SS_FIELDS_MERGE */
    uint64_t first, last;                   /* last 0: to the line's end */
    uint64_t flags;
    uint64_t members;                       /* byte values in the set */
    uint64_t accepts_delimiter;             /* 1: the set holds the delimiter asked about (it never separates) */
} ss_fields_stats;

SS_API int ss_fields_new(const uint64_t *set, int mode, uint64_t first, uint64_t last, unsigned flags, ss_fields **fields);
SS_API void ss_fields_free(ss_fields *fields);
SS_API int ss_fields_info(const ss_fields *fields, int delimiter, ss_fields_stats *stats);
SS_API int ss_fields_parse(const char *text, uint64_t *first, uint64_t *last);
SS_API int ss_count_fields_device(const ss_fields *fields, const void *d_haystack, size_t len, int delimiter, void *hip_stream,
                                  uint64_t *lines_selected, uint64_t *lines_total);
SS_API int ss_find_fields_device(const ss_fields *fields, const void *d_haystack, size_t len, int delimiter, void *hip_stream,
                                 uint64_t *d_begin, uint64_t *d_end, uint64_t *d_number, uint64_t capacity, uint64_t *total);

#ifdef __cplusplus
}
#endif
#endif /* SLICESLICE_HIP_FIELDS_H */
