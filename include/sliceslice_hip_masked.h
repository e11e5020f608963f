/* sliceslice_hip_masked.h - byte patterns with wildcards and per-byte masks, searched in ONE pass over the haystack: YARA / ClamAV
 * hex strings (`48 8B ?? ?? 89 4?`), a `.` inside a literal, `[0-9][0-9][0-9]` as one nibble mask per byte, a needle whose letters
 * may be in either case.  An OPT-IN component shipped in a library of its own.
 *
 *   libsliceslice_hip_masked.so  the leftmost library's objects PLUS the masked scan (sliceslice-rs_amd/csrc/ss_masked.hip):
 *                                every function of sliceslice_hip_leftmost.h and of the headers it includes, and those below.
 *                                Linked INSTEAD of libsliceslice_hip.so; searchers, sets and patterns belong to the library that
 *                                made them.
 *
 * THE RULE (everything else refers to it):
 *   Pattern     n bytes of `value` and n bytes of `mask`, 1 <= n <= SS_MASKED_MAX_LEN (4,096: both arrays are staged in 8 KiB of
 *               LDS).  A longer pattern and n == 0 are refused.  `value` is stored as value & mask.
 *   Occurrence  every p in [0, len - n] with (hay[p + i] & mask[i]) == value[i] for all i < n.  Occurrences overlap and are counted
 *               as ss_count_device counts them.  Bytes outside [0, len) are absent, whatever memory holds there, and no load touches
 *               a 16-byte block that holds no byte of the view.  Offsets, counts and lengths are 64-bit.
 *   Wildcards   a pattern whose masks are all zero is valid: it matches at every p, so its count is len - n + 1 when n <= len.
 *   Lines       a line matches when an occurrence lies wholly inside it.  An occurrence whose bytes include the delimiter lies in
 *               no line, even where a wildcard position accepts the delimiter's value: `61 ?? 62` does not match "a\nb".  The
 *               delimiter, the last line and the record layout (begin, end, number), ascending, are sliceslice_hip_lines.h's,
 *               word for word.
 *
 *   ss_masked_new            value, mask (host memory, n bytes each; a NULL mask means all 0xFF) -> a pattern on the current device.
 *                            The pattern keeps its device tables the way ss_needle_set_new keeps a set's.
 *   ss_masked_free           NULL is allowed.
 *   ss_masked_info           n, the filter's anchor position and distance (below), the number of bytes with mask 0xFF / partial /
 *                            0x00, and whether any position accepts `delimiter` (0 .. 255; a negative one asks for nothing).
 *   ss_masked_parse_hex      HOST ONLY.  Tokens of two characters separated by optional blanks (space, tab); each character is a hex
 *                            digit of either case or `?`: `4?`, `?F` and `??` are all valid.  value[k] / mask[k] of token k are
 *                            written for k < capacity (either array may be NULL) and *n is the number of tokens.  Anything else is
 *                            refused with the offending column (from 1) in ss_last_error; an empty text gives n == 0.
 *   ss_masked_choose_filter  HOST ONLY: the choice the constructor makes.  The kernel tests TWO pattern positions in registers,
 *                            `anchor` and `anchor + distance` with 0 <= distance <= 16 (0: one filter byte), and settles what they
 *                            let through by a masked compare in memory.  The cost of a position is the sum, over the byte values it
 *                            accepts, of the per-byte cost ss_choose_filter_triple uses (static rarity classes, or - with a
 *                            histogram of the haystack, 256 counts - the log of the accepted values' summed count) plus one per
 *                            accepted value; the pair with the smallest sum of costs wins, the earliest on ties.  A position whose
 *                            mask is 0x00 is never chosen while any other exists; where only one position has a mask, or all that
 *                            have one are more than 16 apart, distance is 0.
 *   ss_count_masked_device / ss_count_masked_device_async / ss_find_all_masked_device
 *                            the argument lists, waits and capacity rules of ss_count_device, ss_count_device_async and
 *                            ss_find_all_device (sliceslice_hip_matches.h).  The async form takes a device result, is stream-ordered,
 *                            needs no scratch and can be captured into a hipGraph.  find_all writes the first min(total, capacity)
 *                            offsets ascending and nothing at index `capacity` or beyond.
 *   ss_count_lines_masked_device / ss_find_lines_masked_device
 *                            the arguments of ss_count_lines_device and ss_find_lines_device (sliceslice_hip_lines.h).
 * Refused with SS_ERR_ARGUMENT and a message, nothing written: a NULL pattern, `value` or result pointer; n out of range; a NULL
 * haystack with len > 0; a pattern made on another device than the current one; a capturing stream in the calls that wait (all but
 * the async count); NULL offsets with a non-zero capacity; a delimiter that is no byte.
 *
 * Cost: ONE scan of the haystack (masked_kernels.hpp: set_all_kernel's geometry; a two-byte masked filter in registers, the second
 * byte from the registers shifted by `distance`; every candidate settled by masked dword compares against value / mask staged once
 * per workgroup in LDS).  Find adds the prefix over one word per workgroup and an emit pass over the workgroups that hold one of
 * the first `capacity` occurrences; no sort, and no global atomic but one add per workgroup to the total.  The output depends on
 * the input alone.  The line calls hand the match mask (one bit at the anchor byte of every occurrence) to the lines library's own
 * chunk, combine and emit passes.  A pattern WITHOUT wildcards is better served by a searcher: DESIGN.md 5.19.
 *
 * Out of scope: variable-length jumps (`[4-6]`); alternatives; word / inverted / context forms; batched, plan, sharded, service and
 * host / file forms; replace; regular expressions.
 */
#ifndef SLICESLICE_HIP_MASKED_H
#define SLICESLICE_HIP_MASKED_H

#include "sliceslice_hip_leftmost.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SS_MASKED_MAX_LEN 4096

typedef struct ss_masked ss_masked;

typedef struct ss_masked_stats {
    uint64_t n;
    uint64_t anchor, distance;              /* the filter: pattern positions anchor and anchor + distance */
    uint64_t full, partial, wild;           /* bytes with mask 0xFF / neither / 0x00 */
    uint64_t accepts_delimiter;             /* 1: some position accepts the delimiter asked about */
    uint64_t reserved;
} ss_masked_stats;

SS_API int ss_masked_new(const void *value, const void *mask, size_t n, ss_masked **pattern);
SS_API void ss_masked_free(ss_masked *pattern);
SS_API int ss_masked_info(const ss_masked *pattern, int delimiter, ss_masked_stats *stats);
SS_API int ss_masked_parse_hex(const char *text, uint8_t *value, uint8_t *mask, size_t capacity, size_t *n);
SS_API int ss_masked_choose_filter(const void *value, const void *mask, size_t n, const uint64_t *hist, size_t *anchor, size_t *distance);
SS_API int ss_count_masked_device(const ss_masked *pattern, const void *d_haystack, size_t len, void *hip_stream, uint64_t *count);
SS_API int ss_count_masked_device_async(const ss_masked *pattern, const void *d_haystack, size_t len, void *hip_stream, uint64_t *d_count);
SS_API int ss_find_all_masked_device(const ss_masked *pattern, const void *d_haystack, size_t len, void *hip_stream, uint64_t *d_offsets,
                                     uint64_t capacity, uint64_t *total);
SS_API int ss_count_lines_masked_device(const ss_masked *pattern, const void *d_haystack, size_t len, int delimiter, void *hip_stream,
                                        uint64_t *lines);
SS_API int ss_find_lines_masked_device(const ss_masked *pattern, const void *d_haystack, size_t len, int delimiter, void *hip_stream,
                                       uint64_t *d_begin, uint64_t *d_end, uint64_t *d_number, uint64_t capacity, uint64_t *lines);

#ifdef __cplusplus
}
#endif
#endif /* SLICESLICE_HIP_MASKED_H */
