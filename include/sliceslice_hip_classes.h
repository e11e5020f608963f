/* sliceslice_hip_classes.h - fixed-length patterns of BYTE CLASSES, searched in ONE pass over the haystack: `[0-9]{3}`, `\d\d:\d\d`,
 * `[0-9A-F]{4}H`, `[^a-z]the[^a-z]`, `[Ff]igure \d\d-\d` - the most common kind of `grep -E` and YARA pattern: a sequence of fixed
 * length whose positions are sets of bytes.  An OPT-IN component shipped in a library of its own.
 *
 *   libsliceslice_hip_classes.so  the masked library's objects PLUS the class scan (sliceslice-rs_amd/csrc/ss_classes.hip):
 *                                 every function of sliceslice_hip_masked.h and of the headers it includes, and those below.
 *                                 Linked INSTEAD of libsliceslice_hip.so; searchers, sets and patterns belong to the library that
 *                                 made them.
 *
 * THE RULE (everything else refers to it):
 *   Pattern     n positions, 1 <= n <= SS_CLASSES_MAX_LEN (4,096).  Each position is a non-empty set of byte values, given as 256
 *               bits in four uint64_t words: byte b is bit b & 63 of word b >> 6.  n == 0, a longer pattern and an empty set are
 *               refused.
 *   Occurrence  every p in [0, len - n] with hay[p + i] in set i for all i < n.  Occurrences overlap and are counted as
 *               ss_count_device counts them.  Bytes outside [0, len) are absent, whatever memory holds there, and no load touches
 *               a 16-byte block that holds no byte of the view.  Offsets, counts and lengths are 64-bit.
 *   Lines       a line matches when an occurrence lies wholly inside it.  An occurrence whose bytes include the delimiter lies in
 *               no line, even where a class accepts the delimiter's value: `a.b` and `a[^x]b` do not match "a\nb".  The
 *               delimiter, the last line and the record layout (begin, end, number), ascending, are sliceslice_hip_lines.h's,
 *               word for word.
 *   Cover       the tightest (value, mask) pair of a set: mask = ~(OR over members c of c ^ c0) for any member c0, value =
 *               c0 & mask, so every member satisfies (c & mask) == value and no pair with more mask bits does.  A position is
 *               SINGLE when its set is one value, MASKED when it has more and is exactly what its cover accepts (`[Ff]`: 46 / DF;
 *               `.`: 00 / 00), INEXACT otherwise (`[0-9]`: 30 / F0 also accepts `:;<=>?`; `[0-9A-F]`: 00 / 88).
 *   Limits      at most SS_CLASSES_MAX_INEXACT (1,024) inexact positions and at most SS_CLASSES_MAX_DISTINCT (64) distinct
 *               inexact sets; a pattern beyond either is refused with SS_ERR_ARGUMENT and a message that names the limit.
 *
 * THE PATTERN LANGUAGE of ss_classes_parse: a strict subset of Python `re` byte patterns under re.DOTALL - whatever is accepted
 * means what `re` means by it.
 *   Outside a set   a literal is any byte other than \ . [ ] { } ( ) * + ? | ^ $ (bytes >= 0x80 are literals); `.` is all 256
 *                   values; the escapes \d \D \w \W \s \S with re's ASCII meanings (\D and \s contain \n), \n \t \r \f \v, \xHH
 *                   with exactly two hex digits, and a backslash before ASCII punctuation, which is that byte.  Every other
 *                   escape is refused: letters, digits, \b, \A, \Z.
 *   Inside [...]    a leading ^ negates.  Items are bytes, the escapes above (class escapes included) and ranges x-y of two single
 *                   bytes with x <= y.  A `-` is a literal only directly after the opening [ or [^, or directly before ].
 *                   Refused: an unescaped [; a ] in first place ([] and [^]); a doubled -- && ~~ ||; a reversed range; a range
 *                   with a class escape as an end; a set that is not closed.
 *   Repetition      {k} directly after an item repeats it k times in total, 1 <= k <= 4096.  {k,} {k,m} {,m} {0} and a { anywhere
 *                   else are refused, and so are ( ) * + ? | ^ $: no groups, variable lengths, alternatives or anchors.
 *   ignore_case     re.I on bytes: the positive set is closed under swapping ASCII case, then negated where ^ says so.  `[^a]`
 *                   does not accept `A`, and `[a-c]` accepts `A`-`C`.
 *   A set that ends up empty (`[^\x00-\xff]`) and more than 4,096 positions are refused.  An empty text gives n == 0, which
 *   ss_classes_new refuses.
 *
 *   ss_classes_new           sets (host memory, 4 words per position) -> a pattern on the current device.  The pattern keeps its
 *                            device tables the way ss_masked_new keeps a pattern's.
 *   ss_classes_free          NULL is allowed.
 *   ss_classes_info          n, the filter's anchor position and distance (ss_masked_choose_filter's rule applied to the covers,
 *                            costing the values the COVER accepts, since that is what the register test lets through), the number
 *                            of single / masked / inexact positions, the number of distinct inexact sets, and whether any set
 *                            accepts `delimiter` (0 .. 255; a negative one asks for nothing).
 *   ss_classes_parse         HOST ONLY: the pattern language above.  The sets of the positions k < capacity are written (`sets` may
 *                            be NULL) and *n is the number of positions.  Anything refused names the offending column (from 1) in
 *                            ss_last_error, as ss_masked_parse_hex does.
 *   ss_classes_cover         HOST ONLY: value[i] / mask[i] of the cover of every position (either array may be NULL).
 *   ss_count_classes_device / ss_count_classes_device_async / ss_find_all_classes_device / ss_count_lines_classes_device /
 *   ss_find_lines_classes_device
 *                            the argument lists, waits, capacity rules and refusals of the five masked calls
 *                            (sliceslice_hip_masked.h), argument for argument, with the pattern first.  The async form takes a
 *                            device result, is stream-ordered, needs no scratch and can be captured into a hipGraph.
 * Refused with SS_ERR_ARGUMENT and a message, nothing written: a NULL pattern, `sets`, text or result pointer; n out of range; an
 * empty set; a pattern beyond one of the two limits; a NULL haystack with len > 0; a pattern made on another device than the
 * current one; a capturing stream in the calls that wait (all but the async count); NULL offsets with a non-zero capacity; a
 * delimiter that is no byte.
 *
 * Cost: ONE scan of the haystack (classes_kernels.hpp, on masked_kernels.hpp's geometry and functions): the masked filter in
 * registers on the covers of two positions, the masked dword compares against the covers staged in LDS, then - for a pattern with
 * inexact positions - the EXACT TEST of every survivor: a check list of (position, set) entries, rarest set first (ascending
 * summed static byte cost of the set's members, ties by position), is walked from LDS against the sets' 32-byte bitmaps in LDS
 * and left at the first miss.  A pattern without inexact positions skips that step and returns what ss_masked_new of its covers
 * returns.  Find and the line calls add what the masked calls add; no sort, no global atomic but one add per workgroup to the
 * total; the output depends on the input alone.  A pattern made ONLY of wide classes (`\w{8}`, `[0-9A-F]{4}`) has covers that
 * accept 128 values, so every ASCII position is a candidate that is settled byte by byte: DESIGN.md 5.20 has the measured rate.
 *
 * Out of scope: variable length (`* + ? {k,m}`); alternatives; groups; anchors; word / inverted / context / batched / replace
 * forms; sharper register filters (two covers per position, SWAR range tests, nibble tables).
 */
#ifndef SLICESLICE_HIP_CLASSES_H
#define SLICESLICE_HIP_CLASSES_H

#include "sliceslice_hip_masked.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SS_CLASSES_MAX_LEN 4096
#define SS_CLASSES_MAX_INEXACT 1024
#define SS_CLASSES_MAX_DISTINCT 64

typedef struct ss_classes ss_classes;

typedef struct ss_classes_stats {
    uint64_t n;
    uint64_t anchor, distance;              /* the filter: pattern positions anchor and anchor + distance */
    uint64_t single, masked, inexact;       /* positions that are one value / more and exactly their cover / the rest */
    uint64_t distinct;                      /* distinct inexact sets */
    uint64_t accepts_delimiter;             /* 1: some set accepts the delimiter asked about */
} ss_classes_stats;

SS_API int ss_classes_new(const uint64_t *sets, size_t n, ss_classes **pattern);
SS_API void ss_classes_free(ss_classes *pattern);
SS_API int ss_classes_info(const ss_classes *pattern, int delimiter, ss_classes_stats *stats);
SS_API int ss_classes_parse(const char *text, int ignore_case, uint64_t *sets, size_t capacity, size_t *n);
SS_API int ss_classes_cover(const uint64_t *sets, size_t n, uint8_t *value, uint8_t *mask);
SS_API int ss_count_classes_device(const ss_classes *pattern, const void *d_haystack, size_t len, void *hip_stream, uint64_t *count);
SS_API int ss_count_classes_device_async(const ss_classes *pattern, const void *d_haystack, size_t len, void *hip_stream, uint64_t *d_count);
SS_API int ss_find_all_classes_device(const ss_classes *pattern, const void *d_haystack, size_t len, void *hip_stream, uint64_t *d_offsets,
                                      uint64_t capacity, uint64_t *total);
SS_API int ss_count_lines_classes_device(const ss_classes *pattern, const void *d_haystack, size_t len, int delimiter, void *hip_stream,
                                         uint64_t *lines);
SS_API int ss_find_lines_classes_device(const ss_classes *pattern, const void *d_haystack, size_t len, int delimiter, void *hip_stream,
                                        uint64_t *d_begin, uint64_t *d_end, uint64_t *d_number, uint64_t capacity, uint64_t *lines);

#ifdef __cplusplus
}
#endif
#endif /* SLICESLICE_HIP_CLASSES_H */
