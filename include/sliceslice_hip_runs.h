/* sliceslice_hip_runs.h - the MAXIMAL RUNS of one byte class, counted and listed in ONE pass over the haystack: `\w+`, `[0-9]+`,
 * `\S+` (what `wc -w` counts), `[0-9]{3,}`, `[A-Z]{2,5}`, ` {2,}`, `[^\n]{80,}` - the variable-length patterns a grep or tokeniser
 * user meets first.  An OPT-IN component shipped in a library of its own.
 *
 *   libsliceslice_hip_runs.so  the classes library's objects PLUS the run scan (sliceslice-rs_amd/csrc/ss_runs.hip): every
 *                              function of sliceslice_hip_classes.h and of the headers it includes, and those below.  Linked
 *                              INSTEAD of libsliceslice_hip.so; searchers, sets and patterns belong to the library that made them.
 *
 * THE RULE (everything else refers to it):
 *   Class       a non-empty set of byte values, given as 256 bits in four uint64_t words: byte b is bit b & 63 of word b >> 6
 *               (sliceslice_hip_classes.h's layout).  The full set is allowed; an empty set is refused.
 *   Run         a maximal interval [begin, end) of the view whose bytes are all in the set: begin == 0 or hay[begin-1] is not in
 *               the set, and end == len or hay[end] is not in the set.  Bytes outside [0, len) are absent, whatever memory holds
 *               there, and no load touches a 16-byte block that holds no byte of the view.
 *   Selected    min_len <= end - begin, and max_len == 0 (no maximum) or end - begin <= max_len.  1 <= min_len <=
 *               SS_RUNS_MAX_LEN (4,096); max_len is 0, or min_len <= max_len <= SS_RUNS_MAX_LEN.  A run that is too long is not
 *               selected, and a run is never chopped into pieces: in `re` terms the selection is (?<![C])[C]{min,max}(?![C]), and
 *               with no maximum it is exactly what re.finditer(rb"[C]{min,}") yields.  Runs cannot overlap, so "overlapping" and
 *               "disjoint" mean the same thing here.
 *   Lines       the delimiter is never a member in the line calls, even where the set holds it, so a run is cut at every
 *               delimiter.  A line matches when it holds a selected run.  The delimiter, the last line and the record layout
 *               (begin, end, number), ascending, are sliceslice_hip_lines.h's.  A set that is only the delimiter matches no line
 *               and is not refused.
 *   Offsets, counts and lengths are 64-bit.
 *
 * THE LANGUAGE of ss_runs_parse: exactly ONE item of the classes language (sliceslice_hip_classes.h: a literal, `.`, an escape, or
 * [...], with the same ignore_case rule) followed by exactly one of `+`, `{k}`, `{k,}`, `{k,m}`.  `+` is (1, none), `{k}` is (k, k),
 * `{k,}` is (k, none), `{k,m}` is (k, m).  Refused, naming the column (from 1) as ss_classes_parse does: `*`, `?`, `{0...}` and
 * `{,m}`, which would match the empty string; a missing quantifier; anything behind the quantifier; k or m above 4,096; m < k.
 *
 *   ss_runs_new              the set (host memory, 4 words), min_len, max_len and flags -> a handle on the current device.
 *                            SS_RUNS_BITMAP forces the bitmap path, so that the two paths can be compared on one set.
 *   ss_runs_free             NULL is allowed.
 *   ss_runs_info             min_len, max_len, the number of members, the number of maximal ranges of the set, the path (0: range
 *                            tests, 1: the bitmap) and whether the set accepts `delimiter` (0 .. 255; a negative one asks for
 *                            nothing).
 *   ss_runs_parse            HOST ONLY: the language above -> the set (4 words), min_len and max_len (0: none).
 *   ss_count_runs_device     the number of selected runs; waits and puts the count in host memory.
 *   ss_count_runs_device_async   stream-ordered: takes a device result, needs no scratch memory and can be captured into a hipGraph.
 *   ss_find_all_runs_device  the first `capacity` selected runs, ascending: d_begin[k] and d_end[k] (either array may be NULL);
 *                            *total is always the full count.  Capacity and NULL rules are ss_find_all_masked_device's.
 *   ss_count_lines_runs_device / ss_find_lines_runs_device
 *                            the argument lists of the two masked line calls, argument for argument, with `runs` first.
 * Refused with SS_ERR_ARGUMENT and a message, nothing written: NULL handles or result pointers; an empty set; lengths out of
 * range; an unknown flag; a NULL haystack with len > 0; a handle made on another device; a capturing stream in the calls that
 * wait; NULL offsets (both arrays) with a non-zero capacity; a delimiter that is no byte.
 *
 * Cost: ONE scan of the haystack (runs_kernels.hpp, on masked_kernels.hpp's geometry and loads).  Membership of every byte is one
 * bit: a set of at most SS_RUNS_MAX_RANGES (4) maximal ranges is tested four bytes per operation by SWAR arithmetic on the dwords
 * (runs_swar.hpp, exact for all 256 values); any other set, or SS_RUNS_BITMAP, reads the 32-byte bitmap in LDS.  Begins and ends
 * are read off the lane's 16-bit mask and one bit of each neighbour.  With min_len == 1 and no maximum every begin is selected: the
 * count is a popcount and no byte is read twice.  Otherwise a begin looks AHEAD at most max(min_len, max_len + 1) bytes and an end
 * looks BACK the same distance: first in registers, on the 32-bit window of the lane's own mask and its neighbour's, where most
 * runs in text end; only a run that reaches the window's edge undecided walks memory from there, never leaves the view and stops
 * at the first non-member.  The total work of the walks is linear in the view, because runs are disjoint; a view made of runs of
 * about min_len bytes is read a second time, one lane per run.  Count: one add per workgroup to the total, the only atomic.  Find:
 * two exclusive prefix sums over the workgroups' begin and end counts, then the same grid again over the workgroups that hold one
 * of the first `capacity` begins or ends; temporary device memory is 32 bytes per workgroup; the output depends on the input alone.
 *
 * Out of scope: more than one item (`[A-Za-z_]\w*`, `\d+\.\d+`); alternatives, groups, anchors; `*` and `?`; chopping long runs
 * the way re's {k,m} does; word / inverted / context / batched / replace forms; counting member bytes or the longest run.
 */
#ifndef SLICESLICE_HIP_RUNS_H
#define SLICESLICE_HIP_RUNS_H

#include "sliceslice_hip_classes.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SS_RUNS_MAX_LEN 4096
#define SS_RUNS_MAX_RANGES 4
#define SS_RUNS_BITMAP 1u

typedef struct ss_runs ss_runs;

typedef struct ss_runs_stats {
    uint64_t min_len, max_len;              /* max_len 0: no maximum */
    uint64_t members;                       /* byte values in the set */
    uint64_t ranges;                        /* maximal ranges of the set */
    uint64_t path;                          /* 0: range tests, 1: the bitmap */
    uint64_t accepts_delimiter;             /* 1: the set accepts the delimiter asked about */
} ss_runs_stats;

SS_API int ss_runs_new(const uint64_t *set, uint64_t min_len, uint64_t max_len, unsigned flags, ss_runs **runs);
SS_API void ss_runs_free(ss_runs *runs);
SS_API int ss_runs_info(const ss_runs *runs, int delimiter, ss_runs_stats *stats);
SS_API int ss_runs_parse(const char *text, int ignore_case, uint64_t *set, uint64_t *min_len, uint64_t *max_len);
SS_API int ss_count_runs_device(const ss_runs *runs, const void *d_haystack, size_t len, void *hip_stream, uint64_t *count);
SS_API int ss_count_runs_device_async(const ss_runs *runs, const void *d_haystack, size_t len, void *hip_stream, uint64_t *d_count);
SS_API int ss_find_all_runs_device(const ss_runs *runs, const void *d_haystack, size_t len, void *hip_stream, uint64_t *d_begin,
                                   uint64_t *d_end, uint64_t capacity, uint64_t *total);
SS_API int ss_count_lines_runs_device(const ss_runs *runs, const void *d_haystack, size_t len, int delimiter, void *hip_stream,
                                      uint64_t *lines);
SS_API int ss_find_lines_runs_device(const ss_runs *runs, const void *d_haystack, size_t len, int delimiter, void *hip_stream,
                                     uint64_t *d_begin, uint64_t *d_end, uint64_t *d_number, uint64_t capacity, uint64_t *lines);

#ifdef __cplusplus
}
#endif
#endif /* SLICESLICE_HIP_RUNS_H */
