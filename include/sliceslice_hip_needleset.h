/* sliceslice_hip_needleset.h - the lines that match any of MANY needles, selected in ONE pass over the haystack (grep -e A -e B,
 * grep -f FILE; with -c, -n, -i, -w, -x, -v and -A / -B / -C).  An OPT-IN component shipped in a library of its own.
 *
 *   libsliceslice_hip_needleset.so  the anyof library's objects PLUS the set scan (sliceslice-rs_amd/csrc/ss_needleset.hip): every
 *                                   function of sliceslice_hip.h, sliceslice_hip_matches.h, sliceslice_hip_lines.h,
 *                                   sliceslice_hip_nocase.h, sliceslice_hip_bounded.h, sliceslice_hip_inverted.h,
 *                                   sliceslice_hip_context.h and sliceslice_hip_anyof.h and the five below.  Linked INSTEAD of
 *                                   libsliceslice_hip.so; searchers and sets belong to the library that made them.
 *
 * Rule:      for the same needles, `how`, `before` and `after` the two set calls return what ss_count_lines_anyof_device and
 *            ss_find_lines_anyof_device return, value for value and array for array (sliceslice_hip_anyof.h has the rule).
 *
 *   ss_needle_set_new       compiles `count` needles (needles[k], lens[k] bytes; a pointer may be NULL where its length is 0) into a
 *                           set on the CURRENT device: sorted and deduplicated, a 256-bit map of the one-byte needles, two 65,536-bit
 *                           maps of the two-byte needles and of the first two bytes of the longer ones, and per two-byte key a bucket
 *                           of {offset, length, bytes 2 .. 5, their mask}.  flags: SS_SET_NOCASE folds 'A'..'Z' of the needles here;
 *                           the calls then fold the haystack's bytes in registers.  The delimiter is never folded.  The needles'
 *                           order, a needle given twice and a needle that is a prefix of another change nothing.
 *   ss_needle_set_info      needles, distinct needles, blob bytes (the needles of three bytes and more), one-byte needles, two-byte
 *                           needles, prefix keys set, the largest bucket, the fold.
 *   ss_count_lines_set_device   *lines = the number of selected lines.
 *   ss_find_lines_set_device    the records of the selected lines with their context, and *selected.
 *   how       SS_BOUND_WORD, SS_BOUND_LINE, SS_CONTEXT_INVERT.  SS_BOUND_NOCASE is accepted only when it equals the set's fold, so
 *             that a caller can pass the anyof call's `how`.
 * Refused with SS_ERR_ARGUMENT, nothing written: a mismatch of SS_BOUND_NOCASE with the set's fold; NULL arguments; count == 0;
 * count > SS_ANYOF_MAX_NEEDLES; a blob of 2^32 bytes or more (checked on the lengths as given: needles whose lengths sum to 2^32 or
 * more are refused even where duplicates or short needles would leave a smaller blob); unknown bits in `flags` or `how`; SS_BOUND_WORD together with
 * SS_BOUND_LINE; the empty needle under either, as the models refuse it; a delimiter outside 0 .. 255; a capturing stream; a set
 * made on another device than the current one.  A failed allocation returns SS_ERR_NOMEM or SS_ERR_HIP with nothing written; the
 * temporary memory is returned on every way out.  Both calls wait for the stream; there is no async form.
 *
 * Cost: the count is ONE scan of the haystack (set_scan_kernel: every position's two-byte key is looked up in both bitmaps with one
 * LDS load; one-byte and two-byte needles match there, longer ones walk a bucket, one masked dword compare per entry before any
 * byte loop; a lane leaves a line alone once it is known to match) plus the line combine of sliceslice_hip_lines.h over one
 * summary per workgroup.  Find with before == after == 0 adds an emit pass over the workgroups that close one of the first
 * `capacity` selected lines and writes (begin, end, number) straight into the caller's arrays, inverted or not; kind is 1.  Find
 * with context lets the emit pass write the selected numbers into ONE temporary buffer sized from the count and hands it to
 * ss_lines_around_device; that route allocates and frees the buffer inside the call (which synchronises the device), waits for
 * the stream after the count, and runs the small combine launches a second time.  A candidate's bucket walk reads the haystack
 * bytes behind its key from memory again, lane by lane.  An empty needle in the set selects every line (none with SS_CONTEXT_INVERT) without a scan beyond the
 * delimiters.  No global atomic, deterministic output, scratch per workgroup only.  Rates measured on an MI355X are in
 * DESIGN.md 5.14.
 *
 * Out of scope: async and capturable forms; batched, plan, sharded, service and host / file forms; -m; -o; a `how` per needle;
 * regular expressions; multi-byte terminators; an occurrence (non-line) form for sets (sliceslice_hip_setmatches.h has it, in a
 * library of its own); the text of the lines (sliceslice_hip_output.h gathers and numbers the records of any line call on the
 * device).
 */
#ifndef SLICESLICE_HIP_NEEDLESET_H
#define SLICESLICE_HIP_NEEDLESET_H

#include "sliceslice_hip_anyof.h"

#define SS_SET_NOCASE 1u                /* ss_needle_set_new flags: the needles are compared ignoring ASCII case */

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ss_needle_set ss_needle_set;

typedef struct ss_needle_set_stats {
    uint64_t needles;                   /* as given */
    uint64_t distinct;                  /* after the fold */
    uint64_t blob_bytes;                /* bytes of the needles of three bytes and more */
    uint64_t one_byte;
    uint64_t two_byte;
    uint64_t prefix_keys;               /* two-byte keys that begin a needle of three bytes or more */
    uint64_t largest_bucket;            /* needles behind the fullest of those keys */
    uint64_t fold;                      /* 1: SS_SET_NOCASE */
} ss_needle_set_stats;

SS_API int ss_needle_set_new(const void *const *needles, const size_t *lens, uint32_t count, unsigned flags, ss_needle_set **out);
SS_API void ss_needle_set_free(ss_needle_set *set);
SS_API int ss_needle_set_info(const ss_needle_set *set, ss_needle_set_stats *stats);
SS_API int ss_count_lines_set_device(const ss_needle_set *set, const void *d_haystack, size_t len, int delimiter, unsigned how,
                                     void *hip_stream, uint64_t *lines);
SS_API int ss_find_lines_set_device(const ss_needle_set *set, const void *d_haystack, size_t len, int delimiter, unsigned how,
                                    uint64_t before, uint64_t after, void *hip_stream, uint64_t *d_begin, uint64_t *d_end,
                                    uint64_t *d_number, uint8_t *d_kind, uint64_t capacity, uint64_t *lines, uint64_t *selected);

#ifdef __cplusplus
}
#endif
#endif /* SLICESLICE_HIP_NEEDLESET_H */
