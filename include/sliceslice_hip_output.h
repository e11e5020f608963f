/* sliceslice_hip_output.h - grep's OUTPUT, written on the device: the text of a list of ranges gathered into one buffer, each with
 * its line number, `:` or `-`, its terminator and the `--` separators of context output (grep -n -A / -B / -C -F needle file,
 * grep -o, sed -n 'Np').  An OPT-IN component shipped in a library of its own.
 *
 *   libsliceslice_hip_output.so  the disjoint library's objects PLUS the size, start and copy kernels
 *                                (sliceslice-rs_amd/csrc/ss_output.hip): every function of sliceslice_hip_disjoint.h and of the
 *                                headers it includes, and the three below.  Linked INSTEAD of libsliceslice_hip.so; searchers
 *                                belong to the library that made them.
 *
 * Rule:      record i - (begin[i], end[i], number[i], kind[i]), what the line calls return - contributes, in this order:
 *              1. with SS_OUTPUT_SEPARATOR, and i > 0, and number[i] > number[i-1] + 1: the two bytes `--` and the terminator;
 *              2. with SS_OUTPUT_NUMBER: the decimal digits of number[i] - a uint64, no leading zeros, 1 to 20 digits, 0 prints
 *                 `0` - followed by `:` when kind[i] != 0 or d_kind is NULL, else by `-`;
 *              3. the bytes [b, e) of the view, where e = min(end[i], len) and b = min(begin[i], e).  Nothing outside the view is
 *                 ever copied, whatever the records say;
 *              4. the terminator byte, when `terminator` is 0..255.  -1 means none, and then the separator is `--` alone.
 *            The output is the concatenation over i = 0 .. count-1.  Records may overlap, repeat or descend: a gather is defined
 *            for any list.  The numbers are unsigned and the comparison of 1. is made without wrapping: it is false where the
 *            numbers descend or repeat (a descending pair gets no separator) and where number[i-1] is 2^64 - 1.
 *            d_starts[i] is the output offset where record i's contribution begins, separator included; d_starts[count] equals
 *            *out_len.  Everything is 64-bit.
 *
 *   ss_format_lines_device   `s` names the device and its scratch only; its needle is never looked at.  *out_len is always set and
 *                            d_starts (count + 1 entries) is written whenever it is non-NULL.  If out_capacity < *out_len, nothing
 *                            is written to d_out and the call returns SS_OK: the caller sizes the buffer and calls again (the
 *                            precedent of ss_replace_device).  Otherwise d_out[0, *out_len) holds the output and nothing is written
 *                            at *out_len or beyond.  d_out may have any alignment.  count == 0 gives 0 with no launch.  Waits for
 *                            the stream.
 *   ss_gather_ranges_device  the same launches with flags == 0 and no numbers: the primitive of grep -o-like and sed -n 'Np'-like
 *                            callers.
 *   ss_grep_lines_device     ss_find_lines_context_device with all four arrays into temporary device memory of 25 bytes per
 *                            printed line (that call's own precedent for temporary memory; returned inside the call), then the
 *                            format with terminator = delimiter.  `how` takes the bits ss_find_lines_context_device takes,
 *                            SS_CONTEXT_INVERT included; its refusals are passed through.  A capacity that is too short still
 *                            reports *out_len, *lines and *selected.  Waits for the stream.
 * Refused with SS_ERR_ARGUMENT and a message that says why, nothing written: unknown flag bits; a terminator outside -1..255;
 * SS_OUTPUT_NUMBER or SS_OUTPUT_SEPARATOR with a NULL d_number, and a NULL d_begin / d_end, with count > 0; a NULL out_len; count >= 2^48;
 * a d_out range that intersects the haystack's range; a NULL d_out where the output fits the capacity and holds a byte; a capturing
 * stream.  A failed temporary allocation returns SS_ERR_NOMEM or SS_ERR_HIP.
 *
 * Cost: four launches.  output_sizes_kernel, one workgroup per SS_OUTPUT_BLOCK records, stores each block's bytes; prefix_kernel
 * ranks the blocks (scratch: 16 bytes per block); output_starts_kernel scans inside the block and writes 8 bytes per record into
 * d_starts, or into temporary device memory where the caller passes NULL; output_copy_kernel runs over the OUTPUT, one workgroup per
 * SS_OUTPUT_CHUNK bytes cut at multiples of that size from the 16-byte aligned address at or below d_out, so that one line of 1 GiB
 * and millions of short ones are spread over the machine alike.  Every lane owns 16-byte aligned units of the output: a unit inside
 * one record's text is one 16-byte load from the view and ONE 16-byte store; a unit that holds a border, digits, a separator or a
 * terminator is composed in registers and stored once; only the units cut by d_out's own first and last byte are stored byte by
 * byte.  Every output byte is stored exactly once, no load touches a 16-byte block that holds no byte of the view, no workgroup waits
 * for another, there is no global atomic and the output depends on the input alone.  Design and measurements: DESIGN.md 5.17.
 *
 * Out of scope: -m; -b byte-offset prefixes; file-name prefixes; colour; a first-`capacity`-bytes form; async / capturable, batched,
 * plan, sharded, service and host / file forms; multi-byte terminators.
 */
#ifndef SLICESLICE_HIP_OUTPUT_H
#define SLICESLICE_HIP_OUTPUT_H

#include "sliceslice_hip_disjoint.h"

#define SS_OUTPUT_NUMBER 1u         /* flags: `number:` / `number-` in front of every record's text */
#define SS_OUTPUT_SEPARATOR 2u      /* flags: `--` wherever two consecutive numbers differ by more than 1 */
#define SS_OUTPUT_BLOCK 4096u       /* records per workgroup of the size passes */
#define SS_OUTPUT_CHUNK 16384u      /* output bytes per workgroup of the copy pass */

#ifdef __cplusplus
extern "C" {
#endif

SS_API int ss_format_lines_device(const ss_searcher *s, const void *d_haystack, size_t len, const uint64_t *d_begin,
                                  const uint64_t *d_end, const uint64_t *d_number, const uint8_t *d_kind, uint64_t count, int terminator,
                                  unsigned flags, void *hip_stream, void *d_out, uint64_t out_capacity, uint64_t *d_starts,
                                  uint64_t *out_len);
SS_API int ss_gather_ranges_device(const ss_searcher *s, const void *d_haystack, size_t len, const uint64_t *d_begin,
                                   const uint64_t *d_end, uint64_t count, int terminator, void *hip_stream, void *d_out,
                                   uint64_t out_capacity, uint64_t *d_starts, uint64_t *out_len);
SS_API int ss_grep_lines_device(const ss_searcher *s, const void *d_haystack, size_t len, int delimiter, unsigned how, uint64_t before,
                                uint64_t after, unsigned flags, void *hip_stream, void *d_out, uint64_t out_capacity, uint64_t *out_len,
                                uint64_t *lines, uint64_t *selected);

#ifdef __cplusplus
}
#endif
#endif /* SLICESLICE_HIP_OUTPUT_H */
