/* sliceslice_hip_groups.h - EQUAL TOKENS OR LINES GROUPED AND COUNTED on the device: `grep -oE '\w+' | sort | uniq -c`,
 * `sort | uniq -c`, `awk '!seen[$0]++'`, a word-frequency table for a vocabulary nobody knows beforehand, dictionary encoding of a
 * column.  The answer is one (first, count) row per distinct key, in the order of a Python dict filled in input order, and
 * optionally the group of every range.  An OPT-IN component shipped in a library of its own.
 *
 *   libsliceslice_hip_groups.so  the fields library's objects PLUS the grouping (sliceslice-rs_amd/csrc/ss_groups.hip): every
 *                                function of sliceslice_hip_fields.h and of the headers it includes, and those below.  Linked
 *                                INSTEAD of libsliceslice_hip.so; handles belong to the library that made them.
 *
 * THE RULE (everything else refers to it):
 *   Key         the key of range k is the bytes hay[begin[k], end[k]).  The ranges come as two 64-bit device arrays; they may
 *               overlap, repeat and descend, and they are clamped to the view exactly as ss_gather_ranges_device
 *               (sliceslice_hip_output.h) clamps them.  With SS_GROUPS_NOCASE every key byte goes through the ASCII fold of
 *               sliceslice_hip_nocase.h ('A'..'Z' become 'a'..'z', every other byte value stays) before it is hashed or compared;
 *               the haystack is not copied.
 *   Equal       two keys are equal when they have the same length and the same bytes.  All empty keys are equal to each other.
 *   Groups      the groups are the classes of equal keys.  Group j is the j-th group in order of its FIRST member, the smallest k:
 *               the order of a Python dict or Counter filled in input order.  first[j] is that k, count[j] is the number of
 *               members, group[k] is the j of range k.
 *   Every output is a function of the input alone: it is bit-identical from run to run, whatever the hardware does inside.
 *   n <= SS_GROUPS_MAX_RANGES (2^32 - 2), because slots and indices are 32-bit inside.  Bytes outside [0, len) are absent,
 *   whatever memory holds there, and no load touches a 16-byte block that holds no byte of the view.  Offsets, indices and counts
 *   are 64-bit in the results.
 *
 * Argument conventions are sliceslice_hip_runs.h's.
 *   ss_group_ranges_device   d_first[j] and d_count[j] for the first `capacity` groups (either may be NULL, and both); d_group, if
 *                            given, holds all n entries whatever the capacity; *groups is always the full number.  n == 0 is
 *                            allowed and gives 0 groups.  Waits for the stream.
 *   ss_group_runs_device     tokenises with a handle of sliceslice_hip_runs.h - ss_find_all_runs_device, counted and then listed
 *                            into the call's own memory - and groups the runs in one call: d_begin[j] and d_end[j] are the FIRST
 *                            token of group j, d_count[j] its members (each array may be NULL); *tokens = the runs.
 *                            ss_gather_ranges_device on (d_begin, d_end) then prints the vocabulary without a host copy.
 *   ss_group_lines_device    the keys are the lines of sliceslice_hip_lines.h without their delimiters: empty lines are included,
 *                            the last line counts only if it has bytes.  d_number[j] is the number of the first line of group j.
 *                            The line records come from the field scan (sliceslice_hip_fields.h: SS_FIELDS_EACH, first 1, last 0,
 *                            SS_FIELDS_KEEP_SHORT - one record per line that spans the whole line).  *lines = the lines.
 *   ss_groups_scratch_bytes  HOST ONLY: the temporary device memory a call over n ranges takes from the library's pool:
 *                            32 + 12 n + 8 T + 12 B bytes, with T = the table's slots, the smallest power of two >= 2 n (at
 *                            least 2; 0 for n == 0) but never more than 2^32 - so above 2^31 ranges T is below 2 n and still
 *                            above n - and B = ceil(n / SS_GROUPS_BLOCK).  That is 8 bytes of hash and
 *                            4 bytes of slot number per range, 4 bytes of slot and 4 bytes of counter per slot, 12 bytes per rank
 *                            block and 32 bytes of totals: 28 to 44 bytes per range up to 2^31 ranges, fewer above.  The run and the
 *                            line form take 16 bytes per range more, for the records they group.  THE POOL KEEPS WHAT IT TOOK: the
 *                            buffers are those of the find-all calls' pool, which hands a call the first free buffer that is
 *                            large enough and never frees one, and here they are gigabytes, not kilobytes: 1 GiB of text is
 *                            about 10 GiB of scratch.  A process that groups inputs of growing size keeps every earlier
 *                            buffer until it ends; group the largest input first where that matters.  A call that fails
 *                            behind its launches keeps its buffer out of the pool.
 *   SS_GROUPS_WEAK_HASH      FOR TESTS: the hash is replaced by length & 3, so every key lands in one of four probe chains.  The
 *                            results are the same with and without it; it is the only way to put long chains, equal hashes with
 *                            unequal bytes and lost compare-and-swaps under test at small sizes.
 * Refused with SS_ERR_ARGUMENT and a message, nothing written and the results left alone: NULL result pointers; NULL arrays with
 * n > 0; a NULL haystack with len > 0; an unknown flag; n above SS_GROUPS_MAX_RANGES (the message names the limit); a delimiter
 * that is no byte; a NULL handle or a handle made on another device; a capturing stream.
 *
 * Cost (groups_kernels.hpp): no sort and no list of candidate pairs.  HASH: 64 bits per range, stored, so that no key is hashed
 * twice; aligned dword loads shifted together in registers, the fold applied there; one lane per key up to SS_GROUPS_LANE_MAX
 * (128) bytes, the whole wave on one key above that.  INSERT: open addressing with linear probing; a slot holds the index of a
 * member of its group or is empty; an empty slot is taken by one compare-and-swap, an occupied one is compared - stored hashes
 * first, bytes only when they agree - and joined by an atomic min, so that it ends up holding the group's first member whatever
 * the arrival order; no lane ever waits for another and slots never become empty again.  COUNT: one add per member, combined
 * inside the wave by a ballot loop over equal slots and then inside the workgroup, over a block of SS_GROUPS_BLOCK ranges, in a
 * workgroup-private LDS table keyed by slot (SS_GROUPS_LDS_BYTES = 24,576 bytes: 2,048 entries of 12), flushed with one add per
 * entry.  RANK AND EMIT: first-member flags per block of SS_GROUPS_BLOCK ranges, the
 * prefix kernel of the find-all calls over the blocks, every first member writes its row at its rank, a last pass writes group[k].
 * The key bytes are read at random: the call is bound by memory transactions, not by bytes.
 *
 * Out of scope: sorting the groups by key bytes (`sort`) - sort the rows you get; grouping by a field of each line; an async or
 * capturable form; batched forms; multi-GPU; folding beyond ASCII; more than 2^32 - 2 ranges.
 */
#ifndef SLICESLICE_HIP_GROUPS_H
#define SLICESLICE_HIP_GROUPS_H

#include "sliceslice_hip_fields.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SS_GROUPS_NOCASE 1u
#define SS_GROUPS_WEAK_HASH 2u
#define SS_GROUPS_MAX_RANGES 0xfffffffeull  /* 2^32 - 2 */
#define SS_GROUPS_BLOCK 4096                /* ranges per rank block */
#define SS_GROUPS_LANE_MAX 128              /* the longest key one lane hashes and compares alone */
#define SS_GROUPS_LDS_BYTES 24576           /* the count kernel's workgroup-private table */

SS_API int ss_group_ranges_device(const void *d_haystack, size_t len, const uint64_t *d_begin, const uint64_t *d_end, uint64_t n,
                                  unsigned flags, void *hip_stream, uint64_t *d_first, uint64_t *d_count, uint64_t capacity,
                                  uint64_t *d_group, uint64_t *groups);
SS_API int ss_group_runs_device(const ss_runs *runs, const void *d_haystack, size_t len, unsigned flags, void *hip_stream,
                                uint64_t *d_begin, uint64_t *d_end, uint64_t *d_count, uint64_t capacity, uint64_t *groups,
                                uint64_t *tokens);
SS_API int ss_group_lines_device(const void *d_haystack, size_t len, int delimiter, unsigned flags, void *hip_stream, uint64_t *d_begin,
                                 uint64_t *d_end, uint64_t *d_number, uint64_t *d_count, uint64_t capacity, uint64_t *groups,
                                 uint64_t *lines);
SS_API int ss_groups_scratch_bytes(uint64_t n, uint64_t *bytes);

#ifdef __cplusplus
}
#endif
#endif /* SLICESLICE_HIP_GROUPS_H */
