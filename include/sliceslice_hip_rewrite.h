/* sliceslice_hip_rewrite.h - the selected RUNS of one byte class REPLACED OR DELETED on the device, in two passes over the
 * haystack and with no list of runs in between: `tr -d '\r'`, `tr -s ' '`, `sed -E 's/[0-9]+/N/g'`, `sed -E 's/[[:space:]]+/ /g'`,
 * "strip every token of 2 to 5 word bytes", "blank out lines longer than 80 bytes".  An OPT-IN component shipped in a library of its
 * own.
 *
 *   libsliceslice_hip_rewrite.so  the runs library's objects PLUS the rewrite (sliceslice-rs_amd/csrc/ss_rewrite.hip): every function
 *                                 of sliceslice_hip_runs.h and of the headers it includes, and the one below.  Linked INSTEAD of
 *                                 libsliceslice_hip.so; searchers, sets and patterns belong to the library that made them.
 *
 * THE RULE (everything else refers to it):
 *   `runs` is a handle of sliceslice_hip_runs.h; its Class, Run and Selected are that header's, word for word.
 *   Delimiter   -1 (none) or a byte 0 .. 255.  With a byte, that byte is never a member in this call, even where the set holds it,
 *               so a run is cut at every delimiter and a delimiter is always copied: the line calls' rule, and what makes
 *               `s/\s+/ /g` behave as sed does, line by line.
 *   Output      the view with every selected run replaced by the `replacement_len` bytes of `replacement`; everything else is
 *               copied in order: non-members, and runs too short or too long to be selected.  A replacement is not rescanned.
 *   *count      the number of selected runs: what ss_count_runs_device returns, or with a delimiter, the count of the pattern
 *               with that byte taken out of its set.
 *   *out_len    len - (sum of the selected runs' lengths) + count * replacement_len, in 64 bits.
 *   In `re` terms d_out[0, *out_len) is re.sub(rb"(?<![C])[C]{min,max}(?![C])", replacement, view); with no maximum that is
 *   re.sub(rb"[C]{min,}", replacement, view).  replacement_len == 0 deletes.
 *   Bytes outside [0, len) are absent, and no load touches a 16-byte block that holds no byte of the view.
 *
 *   ss_replace_runs_device   `replacement` is HOST memory (at most SS_REWRITE_MAX_TEXT bytes).  *out_len and *count are always set
 *                            on SS_OK.  If out_capacity < *out_len nothing is written and the call returns SS_OK: a NULL d_out
 *                            with capacity 0 is the sizing call, ONE pass.  Otherwise every byte of d_out[0, *out_len) is written
 *                            exactly once, and nothing at *out_len or beyond.  The call waits for the stream.  len == 0 gives 0, 0
 *                            with no launch.
 * Refused with SS_ERR_ARGUMENT and a message, nothing written: a NULL handle or result pointers; a NULL haystack with len > 0; a
 * delimiter outside -1 .. 255; a set that is only the delimiter (nothing can match); a NULL replacement with replacement_len > 0;
 * replacement_len > SS_REWRITE_MAX_TEXT; a NULL d_out with out_capacity > 0; a d_out range that intersects the haystack's range
 * (the rewrite is not made in place); an overflow of *out_len; a capturing stream; a handle made on another device.
 *
 * Cost: the run kernels' geometry, loads, view edges, membership and begin / end selection, called (runs_kernels.hpp): 16 B per
 * lane, 1 KiB per piece, 4 KiB per wave, 16 KiB per tile, 128 KiB per workgroup.  With a delimiter that the set accepts the call
 * takes the bitmap path with that bit cleared.  SIZE PASS: every workgroup leaves three 64-bit words, taken mod 2^64 - its selected
 * begins, its selected ends and S = sum(e + 1) - sum(b) over them in view coordinates - followed by three exclusive prefix sums.
 * For a workgroup whose first byte is view position P: open = rank_b - rank_e (0 or 1: a selected run is open at P), the bytes
 * removed in front of it are PS + open * P, and its output begins at P - (PS + open * P) + rank_b * replacement_len.  The three
 * totals give *count and *out_len.  WRITE PASS (skipped when out_capacity is too small): the same grid; a lane's inside mask is the
 * prefix-XOR of its begins and ends, keep = valid & ~inside, and exclusive sums over lanes, pieces, waves and tiles place its
 * popcount(keep) + popcount(begins) * replacement_len bytes.  A replacement is written where its run begins, by the workgroup that
 * holds the begin, from a copy staged in LDS.  A lane that keeps all 16 of its bytes and begins no run makes ONE 16-byte store;
 * other lanes store byte by byte; a text above 16 bytes is copied by the whole wave, one begin at a time.  No waiting between
 * workgroups, no atomic; temporary device memory is 48 bytes per workgroup plus a constant, never per run; the output depends on
 * the input alone.
 *
 * Out of scope: an async / capturable form; back-references; per-run texts; more than one item; anchors; batched forms; a plain
 * byte translate (`tr a-z A-Z`).
 */
#ifndef SLICESLICE_HIP_REWRITE_H
#define SLICESLICE_HIP_REWRITE_H

#include "sliceslice_hip_runs.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SS_REWRITE_MAX_TEXT 4096

SS_API int ss_replace_runs_device(const ss_runs *runs, const void *d_haystack, size_t len, int delimiter, const void *replacement,
                                  size_t replacement_len, void *hip_stream, void *d_out, uint64_t out_capacity, uint64_t *out_len,
                                  uint64_t *count);

#ifdef __cplusplus
}
#endif
#endif /* SLICESLICE_HIP_REWRITE_H */
