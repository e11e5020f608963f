"""Python host-side mirror of the reference's searcher interface over the C ABI.

Names and argument meaning follow the reference (all paths under /root/reference):

    DynamicHipSearcher.new(needle)                  DynamicAvx2Searcher::new            src/x86.rs:454
    DynamicHipSearcher.with_position(needle, pos)   DynamicAvx2Searcher::with_position  src/x86.rs:468
    HipSearcher.new / .with_position                Avx2Searcher::new / ::with_position src/x86.rs:282,297
    MemchrHipSearcher.new(byte)                     MemchrSearcher::new                 src/lib.rs:124
    searcher.search_in(haystack) -> bool            DynamicAvx2Searcher::search_in      src/x86.rs:523
    PositionError                                   the `assert!` panics                src/x86.rs:300,473

``search_in`` accepts a CUDA/HIP ``torch.Tensor`` of dtype uint8 (device path, no copy), a raw
``(device_pointer, length)`` pair, or host bytes / bytearray / numpy uint8 (uploaded, then scanned on
the GPU).  There is no CPU search path: if the HIP library cannot be loaded, or no GPU is visible,
construction raises.

PyTorch is used only as plumbing (device memory, streams, torch.distributed); the C ABI has no torch
types in its signatures and this module does not import torch unless a tensor is passed in.
"""
import ctypes
import os
import sys

import numpy as np

from . import _build

SS_OK, SS_ERR_POSITION, SS_ERR_ARGUMENT, SS_ERR_NO_DEVICE, SS_ERR_HIP, SS_ERR_RCCL, SS_ERR_NOMEM, SS_ERR_PEER = range(8)

_lib = None

_vp = ctypes.c_void_p
_sz = ctypes.c_size_t
_u64 = ctypes.c_uint64
_int = ctypes.c_int
_pint = ctypes.POINTER(ctypes.c_int)
_pvp = ctypes.POINTER(ctypes.c_void_p)

_psz = ctypes.POINTER(_sz)
_pu64 = ctypes.POINTER(_u64)

# every symbol include/sliceslice_hip.h declares (the product library): name -> (restype, argtypes)
ABI = {
    "ss_searcher_new": (_int, [_vp, _sz, _pvp]),
    "ss_searcher_with_position": (_int, [_vp, _sz, _sz, _pvp]),
    "ss_searcher_free": (None, [_vp]),
    "ss_searcher_info": (_int, [_vp, _psz, _psz]),
    "ss_searcher_filter3": (_int, [_vp, _psz, _psz, _psz]),
    "ss_searcher_set_filter3": (_int, [_vp, _sz, _sz, _sz]),
    "ss_byte_histogram_device": (_int, [_vp, _sz, _sz, _vp, _vp]),
    "ss_choose_position": (_int, [_vp, _sz, _vp, _psz]),
    "ss_choose_filter_triple": (_int, [_vp, _sz, _vp, _psz, _psz, _psz]),
    "ss_search_device": (_int, [_vp, _vp, _sz, _vp, _pint]),
    "ss_search_device_async": (_int, [_vp, _vp, _sz, _vp, _vp]),
    "ss_find_device": (_int, [_vp, _vp, _sz, _vp, _pu64]),
    "ss_find_host": (_int, [_vp, _vp, _sz, _pu64]),
    "ss_find_device_async": (_int, [_vp, _vp, _sz, _u64, _vp, _vp]),
    "ss_search_host": (_int, [_vp, _vp, _sz, _pint]),
    "ss_search_file": (_int, [_vp, ctypes.c_char_p, _pint]),
    "ss_search_batched": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp, _vp]),
    "ss_find_batched": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp, _vp]),
    "ss_batch_plan_create": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _int, _vp, _pvp]),
    "ss_batch_plan_run": (_int, [_vp, _vp, _vp]),
    "ss_batch_plan_free": (None, [_vp]),
    "ss_search_pairs": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp, _vp]),
    "ss_searcher_set_timing": (_int, [_vp, _int]),
    "ss_searcher_last_kernel_ms": (_int, [_vp, ctypes.POINTER(ctypes.c_float)]),
    "ss_searcher_last_launch": (_int, [_vp, _pint, ctypes.POINTER(ctypes.c_uint)]),
    "ss_shard_range": (_int, [_sz, _sz, _int, _int, _psz, _psz]),
    "ss_comm_unique_id": (_int, [_vp]),
    "ss_comm_init_rank": (_int, [_vp, _int, _int, _pvp]),
    "ss_comm_free": (None, [_vp]),
    "ss_comm_count": (_int, [_vp, _pint]),
    "ss_comm_rccl_info": (_int, [ctypes.c_char_p, _sz, _pint]),
    "ss_search_sharded": (_int, [_vp, _vp, _sz, _vp, _vp, _pint]),
    "ss_find_sharded": (_int, [_vp, _vp, _sz, _u64, _vp, _vp, _pu64]),
    "ss_comm_init_all": (_int, [_int, _pint, _pvp]),
    "ss_comm_set_free": (None, [_vp]),
    "ss_comm_set_combine": (_int, [_vp, _int]),
    "ss_comm_set_issue": (_int, [_vp, _int]),
    "ss_comm_set_count": (_int, [_vp, _pint]),
    "ss_comm_set_last_kernel_ms": (_int, [_vp, ctypes.POINTER(ctypes.c_float), _int]),
    "ss_comm_set_last_issue_us": (_int, [_vp, ctypes.POINTER(ctypes.c_float)]),
    "ss_search_sharded_all": (_int, [_vp, _pvp, _psz, _vp, _pint]),
    "ss_find_sharded_all": (_int, [_vp, _pvp, _psz, _pu64, _vp, _pu64]),
    "ss_set_autotune": (_int, [_int]),
    "ss_searcher_tuning_state": (_int, [_vp, _vp, _sz, _vp]),
    "ss_last_error": (ctypes.c_char_p, []),
    "ss_device_info": (_int, [ctypes.c_char_p, _sz, _pint, _psz]),
}
# include/sliceslice_hip_service.h: the resident search service, an opt-in component outside the hot path - NOT in the product
# library: libsliceslice_hip_service.so (the product's objects plus the service) and the hooks builds hold it
SERVICE_ABI = {
    "ss_service_start": (_int, [_int, ctypes.c_double, _pvp]),
    "ss_service_search": (_int, [_vp, _vp, _vp, _sz, _pint]),
    "ss_service_bind": (_int, [_vp, _vp, _sz]),
    "ss_service_stop": (None, [_vp]),
}
# include/sliceslice_hip_matches.h: every occurrence (count, find-all) - NOT in the product library: libsliceslice_hip_matches.so
# (the product's objects plus the all-matches scan) holds it
MATCHES_ABI = {
    "ss_count_device": (_int, [_vp, _vp, _sz, _vp, _pu64]),
    "ss_count_device_async": (_int, [_vp, _vp, _sz, _vp, _vp]),
    "ss_find_all_device": (_int, [_vp, _vp, _sz, _vp, _vp, _u64, _pu64]),
}
# include/sliceslice_hip_matches_batched.h: every occurrence for a batch of problems - libsliceslice_hip_matches_batched.so only (the
# matches library's objects plus the batched all-matches scan)
MATCHES_BATCHED_ABI = {
    "ss_count_batched": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp, _vp]),
    "ss_find_all_batched": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp, _vp, _vp, _vp, _u64, _pu64]),
}
# include/sliceslice_hip_lines.h: the lines that contain a needle (count, records) - libsliceslice_hip_lines.so only (the matches
# library's objects plus the matching-lines scan)
LINES_ABI = {
    "ss_count_lines_device": (_int, [_vp, _vp, _sz, _int, _vp, _pu64]),
    "ss_count_lines_device_async": (_int, [_vp, _vp, _sz, _int, _vp, _vp]),
    "ss_find_lines_device": (_int, [_vp, _vp, _sz, _int, _vp, _vp, _vp, _vp, _u64, _pu64]),
}
# include/sliceslice_hip_nocase.h: every occurrence and the matching lines ignoring ASCII case - libsliceslice_hip_nocase.so only
# (the lines library's objects plus the case-folding scans)
NOCASE_ABI = {
    "ss_searcher_new_nocase": (_int, [_vp, _sz, ctypes.POINTER(ctypes.c_void_p)]),
    "ss_count_nocase_device": (_int, [_vp, _vp, _sz, _vp, _pu64]),
    "ss_count_nocase_device_async": (_int, [_vp, _vp, _sz, _vp, _vp]),
    "ss_find_all_nocase_device": (_int, [_vp, _vp, _sz, _vp, _vp, _u64, _pu64]),
    "ss_count_lines_nocase_device": (_int, [_vp, _vp, _sz, _int, _vp, _pu64]),
    "ss_count_lines_nocase_device_async": (_int, [_vp, _vp, _sz, _int, _vp, _vp]),
    "ss_find_lines_nocase_device": (_int, [_vp, _vp, _sz, _int, _vp, _vp, _vp, _vp, _u64, _pu64]),
}
# include/sliceslice_hip_bounded.h: whole-word / whole-line occurrences and matching lines - libsliceslice_hip_bounded.so only (the
# nocase library's objects plus the bounded scans); the models' argument lists with `unsigned how` in front of the stream
_uint = ctypes.c_uint
BOUNDED_ABI = {
    "ss_count_bounded_device": (_int, [_vp, _vp, _sz, _uint, _vp, _pu64]),
    "ss_count_bounded_device_async": (_int, [_vp, _vp, _sz, _uint, _vp, _vp]),
    "ss_find_all_bounded_device": (_int, [_vp, _vp, _sz, _uint, _vp, _vp, _u64, _pu64]),
    "ss_count_lines_bounded_device": (_int, [_vp, _vp, _sz, _int, _uint, _vp, _pu64]),
    "ss_count_lines_bounded_device_async": (_int, [_vp, _vp, _sz, _int, _uint, _vp, _vp]),
    "ss_find_lines_bounded_device": (_int, [_vp, _vp, _sz, _int, _uint, _vp, _vp, _vp, _vp, _u64, _pu64]),
}
SS_BOUND_WORD, SS_BOUND_LINE, SS_BOUND_NOCASE = 1, 2, 4
# include/sliceslice_hip_inverted.h: the lines that do NOT match - libsliceslice_hip_inverted.so only (the bounded library's objects
# plus the inverted kernels); the line calls' argument lists with `unsigned how` behind the delimiter, as in the bounded line calls
INVERTED_ABI = {
    "ss_count_lines_inverted_device": (_int, [_vp, _vp, _sz, _int, _uint, _vp, _pu64]),
    "ss_count_lines_inverted_device_async": (_int, [_vp, _vp, _sz, _int, _uint, _vp, _vp]),
    "ss_find_lines_inverted_device": (_int, [_vp, _vp, _sz, _int, _uint, _vp, _vp, _vp, _vp, _u64, _pu64]),
}
# include/sliceslice_hip_context.h: matching lines with their context lines, and the records of any set of line numbers -
# libsliceslice_hip_context.so only (the inverted library's objects plus the context kernels)
CONTEXT_ABI = {
    "ss_lines_around_device": (_int, [_vp, _vp, _sz, _int, _vp, _u64, _u64, _u64, _vp, _vp, _vp, _vp, _vp, _u64, _pu64]),
    "ss_find_lines_context_device": (_int, [_vp, _vp, _sz, _int, _uint, _u64, _u64, _vp, _vp, _vp, _vp, _vp, _u64, _pu64, _pu64]),
}
SS_CONTEXT_INVERT = 8
CONTEXT_PART_BYTES = 65536          # SS_CONTEXT_PART_BYTES: bytes of the view per workgroup of the delimiter census
# include/sliceslice_hip_anyof.h: the lines that match any of several needles, and the ordered union of ascending lists of line
# numbers - libsliceslice_hip_anyof.so only (the context library's objects plus the union kernels)
_u32 = ctypes.c_uint32
ANYOF_ABI = {
    "ss_union_numbers_device": (_int, [_vp, _vp, _vp, _u32, _u64, _int, _vp, _vp, _u64, _pu64]),
    "ss_count_lines_anyof_device": (_int, [_vp, _u32, _vp, _sz, _int, _uint, _vp, _pu64]),
    "ss_find_lines_anyof_device": (_int, [_vp, _u32, _vp, _sz, _int, _uint, _u64, _u64, _vp, _vp, _vp, _vp, _vp, _u64, _pu64, _pu64]),
}
ANYOF_MAX_NEEDLES = 65536           # SS_ANYOF_MAX_NEEDLES: needles (or lists) per call
ANYOF_SEGMENT_LINES = 65536         # SS_ANYOF_SEGMENT_LINES: line numbers per workgroup of the union kernels
# include/sliceslice_hip_needleset.h: the lines that match any of many needles in ONE pass over the haystack -
# libsliceslice_hip_needleset.so only (the anyof library's objects plus the set scan)
NEEDLESET_ABI = {
    "ss_needle_set_new": (_int, [_vp, _vp, _u32, _uint, _pvp]),
    "ss_needle_set_free": (None, [_vp]),
    "ss_needle_set_info": (_int, [_vp, _vp]),
    "ss_count_lines_set_device": (_int, [_vp, _vp, _sz, _int, _uint, _vp, _pu64]),
    "ss_find_lines_set_device": (_int, [_vp, _vp, _sz, _int, _uint, _u64, _u64, _vp, _vp, _vp, _vp, _vp, _u64, _pu64, _pu64]),
}
SS_SET_NOCASE = 1
# ss_needle_set_stats: eight 64-bit words, in this order
NEEDLESET_STATS = ("needles", "distinct", "blob_bytes", "one_byte", "two_byte", "prefix_keys", "largest_bucket", "fold")
# include/sliceslice_hip_setmatches.h: every occurrence of every needle of a set, counted per needle and listed as (offset, rank)
# pairs in ONE pass - libsliceslice_hip_setmatches.so only (the needleset library's objects plus the occurrence scan)
SETMATCHES_ABI = {
    "ss_needle_set_ranks": (_int, [_vp, _vp]),
    "ss_count_set_device": (_int, [_vp, _vp, _sz, _uint, _vp, _vp, _pu64]),
    "ss_count_set_device_async": (_int, [_vp, _vp, _sz, _uint, _vp, _vp, _vp]),
    "ss_find_all_set_device": (_int, [_vp, _vp, _sz, _uint, _vp, _vp, _vp, _u64, _pu64]),
}
# include/sliceslice_hip_disjoint.h: the non-overlapping occurrences of a needle (count, offsets, replace) and the greedy selection
# over any ascending list of offsets - libsliceslice_hip_disjoint.so only (the setmatches library's objects plus the selection and
# the replace kernels)
DISJOINT_ABI = {
    "ss_select_disjoint_device": (_int, [_vp, _vp, _u64, _u64, _vp, _vp, _u64, _pu64]),
    "ss_count_disjoint_device": (_int, [_vp, _vp, _sz, _uint, _vp, _pu64]),
    "ss_find_all_disjoint_device": (_int, [_vp, _vp, _sz, _uint, _vp, _vp, _u64, _pu64]),
    "ss_replace_device": (_int, [_vp, _vp, _sz, _uint, _vp, _sz, _vp, _vp, _u64, _pu64, _pu64]),
}
DISJOINT_BLOCK = 4096               # SS_DISJOINT_BLOCK: offsets per workgroup of the selection kernels
# include/sliceslice_hip_output.h: grep's output written on the device (the gather of any list of ranges, with line numbers,
# terminators and `--` separators) - libsliceslice_hip_output.so only (the disjoint library's objects plus the output kernels)
OUTPUT_ABI = {
    "ss_format_lines_device": (_int, [_vp, _vp, _sz, _vp, _vp, _vp, _vp, _u64, _int, _uint, _vp, _vp, _u64, _vp, _pu64]),
    "ss_gather_ranges_device": (_int, [_vp, _vp, _sz, _vp, _vp, _u64, _int, _vp, _vp, _u64, _vp, _pu64]),
    "ss_grep_lines_device": (_int, [_vp, _vp, _sz, _int, _uint, _u64, _u64, _uint, _vp, _vp, _u64, _pu64, _pu64, _pu64]),
}
SS_OUTPUT_NUMBER, SS_OUTPUT_SEPARATOR = 1, 2
OUTPUT_BLOCK = 4096                 # SS_OUTPUT_BLOCK: records per workgroup of the size passes
OUTPUT_CHUNK = 16384                # SS_OUTPUT_CHUNK: output bytes per workgroup of the copy pass
# include/sliceslice_hip_leftmost.h: the leftmost-longest, non-overlapping occurrences of a needle set (count, offsets and needles,
# replace with a text per needle) and that selection over any list of (offset, length) entries - libsliceslice_hip_leftmost.so
# only (the output library's objects plus the selection and the set-replace kernels)
LEFTMOST_ABI = {
    "ss_select_leftmost_device": (_int, [_vp, _vp, _vp, _u64, _vp, _vp, _vp, _u64, _pu64]),
    "ss_count_leftmost_set_device": (_int, [_vp, _vp, _sz, _uint, _vp, _pu64]),
    "ss_find_all_leftmost_set_device": (_int, [_vp, _vp, _sz, _uint, _vp, _vp, _vp, _u64, _pu64]),
    "ss_replace_set_device": (_int, [_vp, _vp, _sz, _uint, _vp, _vp, _u32, _vp, _vp, _u64, _pu64, _pu64]),
    "ss_needle_set_lengths": (_int, [_vp, _vp]),
}
LEFTMOST_BLOCK = 4096               # SS_LEFTMOST_BLOCK: entries per workgroup of the selection kernels
# include/sliceslice_hip_masked.h: byte patterns with wildcards and per-byte masks, searched in ONE pass (occurrences and matching
# lines) - libsliceslice_hip_masked.so only (the leftmost library's objects plus the masked scan)
MASKED_ABI = {
    "ss_masked_new": (_int, [_vp, _vp, _sz, _pvp]),
    "ss_masked_free": (None, [_vp]),
    "ss_masked_info": (_int, [_vp, _int, _vp]),
    "ss_masked_parse_hex": (_int, [ctypes.c_char_p, _vp, _vp, _sz, _psz]),
    "ss_masked_choose_filter": (_int, [_vp, _vp, _sz, _vp, _psz, _psz]),
    "ss_count_masked_device": (_int, [_vp, _vp, _sz, _vp, _pu64]),
    "ss_count_masked_device_async": (_int, [_vp, _vp, _sz, _vp, _vp]),
    "ss_find_all_masked_device": (_int, [_vp, _vp, _sz, _vp, _vp, _u64, _pu64]),
    "ss_count_lines_masked_device": (_int, [_vp, _vp, _sz, _int, _vp, _pu64]),
    "ss_find_lines_masked_device": (_int, [_vp, _vp, _sz, _int, _vp, _vp, _vp, _vp, _u64, _pu64]),
}
MASKED_MAX_LEN = 4096               # SS_MASKED_MAX_LEN: bytes of a pattern
# ss_masked_stats: eight 64-bit words, in this order
MASKED_STATS = ("n", "anchor", "distance", "full", "partial", "wild", "accepts_delimiter", "reserved")
# include/sliceslice_hip_classes.h: fixed-length patterns of byte classes ([0-9], \\w), searched in ONE pass (occurrences and matching
# lines) - libsliceslice_hip_classes.so only (the masked library's objects plus the class scan)
CLASSES_ABI = {
    "ss_classes_new": (_int, [_vp, _sz, _pvp]),
    "ss_classes_free": (None, [_vp]),
    "ss_classes_info": (_int, [_vp, _int, _vp]),
    "ss_classes_parse": (_int, [ctypes.c_char_p, _int, _vp, _sz, _psz]),
    "ss_classes_cover": (_int, [_vp, _sz, _vp, _vp]),
    "ss_count_classes_device": (_int, [_vp, _vp, _sz, _vp, _pu64]),
    "ss_count_classes_device_async": (_int, [_vp, _vp, _sz, _vp, _vp]),
    "ss_find_all_classes_device": (_int, [_vp, _vp, _sz, _vp, _vp, _u64, _pu64]),
    "ss_count_lines_classes_device": (_int, [_vp, _vp, _sz, _int, _vp, _pu64]),
    "ss_find_lines_classes_device": (_int, [_vp, _vp, _sz, _int, _vp, _vp, _vp, _vp, _u64, _pu64]),
}
CLASSES_MAX_LEN = 4096              # SS_CLASSES_MAX_LEN: positions of a pattern
CLASSES_MAX_INEXACT = 1024          # SS_CLASSES_MAX_INEXACT: positions whose set is not exactly its cover
CLASSES_MAX_DISTINCT = 64           # SS_CLASSES_MAX_DISTINCT: distinct sets among them
# ss_classes_stats: eight 64-bit words, in this order
CLASSES_STATS = ("n", "anchor", "distance", "single", "masked", "inexact", "distinct", "accepts_delimiter")
# include/sliceslice_hip_runs.h: the maximal runs of one byte class (\\w+, [0-9]{3,}), counted and listed in ONE pass (runs and
# matching lines) - libsliceslice_hip_runs.so only (the classes library's objects plus the run scan)
RUNS_ABI = {
    "ss_runs_new": (_int, [_vp, _u64, _u64, ctypes.c_uint, _pvp]),
    "ss_runs_free": (None, [_vp]),
    "ss_runs_info": (_int, [_vp, _int, _vp]),
    "ss_runs_parse": (_int, [ctypes.c_char_p, _int, _vp, _pu64, _pu64]),
    "ss_count_runs_device": (_int, [_vp, _vp, _sz, _vp, _pu64]),
    "ss_count_runs_device_async": (_int, [_vp, _vp, _sz, _vp, _vp]),
    "ss_find_all_runs_device": (_int, [_vp, _vp, _sz, _vp, _vp, _vp, _u64, _pu64]),
    "ss_count_lines_runs_device": (_int, [_vp, _vp, _sz, _int, _vp, _pu64]),
    "ss_find_lines_runs_device": (_int, [_vp, _vp, _sz, _int, _vp, _vp, _vp, _vp, _u64, _pu64]),
}
RUNS_MAX_LEN = 4096                 # SS_RUNS_MAX_LEN: the largest min_len / max_len
RUNS_MAX_RANGES = 4                 # SS_RUNS_MAX_RANGES: maximal ranges of a set on the range path
SS_RUNS_BITMAP = 1                  # ss_runs_new flag: force the bitmap path
# ss_runs_stats: six 64-bit words, in this order
RUNS_STATS = ("min_len", "max_len", "members", "ranges", "path", "accepts_delimiter")
# include/sliceslice_hip_rewrite.h: the selected runs of one byte class replaced or deleted on the device (tr -d, sed s/[0-9]+/N/g) -
# libsliceslice_hip_rewrite.so only (the runs library's objects plus the rewrite)
REWRITE_ABI = {
    "ss_replace_runs_device": (_int, [_vp, _vp, _sz, _int, _vp, _sz, _vp, _vp, _u64, _pu64, _pu64]),
}
SS_REWRITE_MAX_TEXT = 4096          # the longest replacement
# include/sliceslice_hip_fields.h: fields first .. last of every line located on the device (cut -f, awk '{print $k}') -
# libsliceslice_hip_fields.so only (the rewrite library's objects plus the field scan)
FIELDS_ABI = {
    "ss_fields_new": (_int, [_vp, _int, _u64, _u64, ctypes.c_uint, _pvp]),
    "ss_fields_free": (None, [_vp]),
    "ss_fields_info": (_int, [_vp, _int, _vp]),
    "ss_fields_parse": (_int, [ctypes.c_char_p, _pu64, _pu64]),
    "ss_count_fields_device": (_int, [_vp, _vp, _sz, _int, _vp, _pu64, _pu64]),
    "ss_find_fields_device": (_int, [_vp, _vp, _sz, _int, _vp, _vp, _vp, _vp, _u64, _pu64]),
}
SS_FIELDS_EACH, SS_FIELDS_MERGE = 0, 1      # ss_fields_new modes: every separator ends a field (cut) / runs of separators do (awk)
SS_FIELDS_KEEP_SHORT = 1            # ss_fields_new flag: an empty record for every line that is not selected
FIELDS_CARRY_CHUNK = 256            # SS_FIELDS_CARRY_CHUNK: workgroup summaries per step of the carry kernel
# ss_fields_stats: six 64-bit words, in this order
FIELDS_STATS = ("mode", "first", "last", "flags", "members", "accepts_delimiter")
# include/sliceslice_hip_groups.h: equal tokens or lines grouped and counted on the device (sort | uniq -c, awk '!seen[$0]++') -
# libsliceslice_hip_groups.so only (the fields library's objects plus the grouping)
GROUPS_ABI = {
    "ss_group_ranges_device": (_int, [_vp, _sz, _vp, _vp, _u64, ctypes.c_uint, _vp, _vp, _vp, _u64, _vp, _pu64]),
    "ss_group_runs_device": (_int, [_vp, _vp, _sz, ctypes.c_uint, _vp, _vp, _vp, _vp, _u64, _pu64, _pu64]),
    "ss_group_lines_device": (_int, [_vp, _sz, _int, ctypes.c_uint, _vp, _vp, _vp, _vp, _vp, _u64, _pu64, _pu64]),
    "ss_groups_scratch_bytes": (_int, [_u64, _pu64]),
}
SS_GROUPS_NOCASE = 1                # flag of the grouping calls: every key byte goes through the ASCII fold
SS_GROUPS_WEAK_HASH = 2             # ... for tests: the hash is length & 3, four probe chains
GROUPS_MAX_RANGES = 2 ** 32 - 2     # SS_GROUPS_MAX_RANGES: ranges of a call
GROUPS_BLOCK = 4096                 # SS_GROUPS_BLOCK: ranges per rank block
GROUPS_LANE_MAX = 128               # SS_GROUPS_LANE_MAX: the longest key one lane hashes and compares alone
GROUPS_LDS_BYTES = 24576            # SS_GROUPS_LDS_BYTES: the count kernel's workgroup-private table
# include/sliceslice_hip_tuning.h, group 1: libsliceslice_hip_tools.so
TOOLS_ABI = {
    "ss_fill_random_device": (_int, [_vp, _u64, _sz, _u64, _vp]),
    "ss_fill_random_host": (_int, [_vp, _u64, _sz, _u64]),
    "ss_read_ceiling": (_int, [_vp, _sz, _vp, _int, ctypes.POINTER(ctypes.c_float)]),
    "ss_selftest_dpp": (_int, [_vp]),
    "ss_tools_last_error": (ctypes.c_char_p, []),
}
# ... group 2: builds with -DSS_TEST_HOOKS only (libsliceslice_hip_tuning.so, the sanitizer builds)
HOOKS_ABI = {
    "ss_version": (ctypes.c_char_p, []),
    "ss_searcher_set_variant": (_int, [_vp, _int]),
    "ss_searcher_set_grid": (_int, [_vp, _int]),
    "ss_choose_filter_for_position": (_int, [_vp, _sz, _sz, _psz, _psz, _psz]),
    "ss_debug_set_epochs": (_int, [_vp, _int]),
    "ss_debug_set_completion_state": (_int, [_vp, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32]),
    "ss_debug_set_comm_epoch": (_int, [_vp, _vp, _int]),
    "ss_debug_late_answers": (_u64, []),
    "ss_debug_fail_next_scans": (_int, [_vp, _int]),
    "ss_debug_census": (_int, [_vp, _vp, _sz, ctypes.POINTER(ctypes.c_uint32)]),
    "ss_debug_census_stats": (_int, [_vp, _vp, _sz, ctypes.POINTER(ctypes.c_uint32), _pint]),
    "ss_debug_plan_filter": (_int, [_vp, _sz, ctypes.POINTER(ctypes.c_uint32)]),
    "ss_debug_plan_cold": (_int, [_vp, _sz, ctypes.POINTER(ctypes.c_uint32)]),
    "ss_debug_plan_layout": (_int, [_vp, ctypes.POINTER(ctypes.c_uint32)]),
    "ss_debug_batch_classes": (_int, [_vp, _vp, _sz, ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint8)]),
    "ss_service_counters": (_int, [_vp, _pu64, _pu64, _pu64]),
}


class TuningState(ctypes.Structure):
    """ss_tuning_state (include/sliceslice_hip.h): every launch-tuning state a handle holds for one haystack."""
    _fields_ = [(k, ctypes.c_uint32) for k in ("autotune", "census_state", "census_age", "tiles", "tiles3", "tiles2", "match_tiles", "lanes",
                                               "pair_lanes", "triple_lanes", "deep_lanes", "triple_state", "on_trial", "trials", "accepted", "settled", "proposal")] + \
               [("own", ctypes.c_uint32 * 3), ("in_force", ctypes.c_uint32 * 3), ("order_measured", ctypes.c_uint32), ("norder", ctypes.c_uint32),
                ("order", ctypes.c_uint8 * 16), ("histogram_state", ctypes.c_uint32), ("workgroups_per_cu", ctypes.c_uint32),
                ("grid", ctypes.c_uint32), ("kernel_mode", ctypes.c_uint32), ("last_found", ctypes.c_uint32)]

    def as_dict(self):
        d = {}
        for k, _ in self._fields_:
            v = getattr(self, k)
            d[k] = list(v) if hasattr(v, "__len__") else int(v)
        d["order"] = d["order"][:d["norder"]]
        return d


def rccl_info():
    """(path of the librccl the native communicators use, its ncclGetVersion) - ss_comm_rccl_info."""
    buf = ctypes.create_string_buffer(512)
    ver = ctypes.c_int(0)
    _check(lib().ss_comm_rccl_info(buf, len(buf), ctypes.byref(ver)))
    return buf.value.decode("utf-8", "replace"), int(ver.value)


def set_autotune(enabled):
    """ss_set_autotune: launch tuning on (the default) or off, process-wide; returns the previous setting."""
    return bool(lib().ss_set_autotune(1 if enabled else 0))


class SlicesliceError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("sliceslice_hip error %d: %s" % (code, msg))
        self.code = code


class PositionError(SlicesliceError, AssertionError):
    """The reference panics here (src/x86.rs:300 `assert!(position < needle.size())`,
    src/x86.rs:473 `assert_eq!(position, 0)`)."""


def _preload_torch():
    if "torch" in sys.modules or os.environ.get("SLICESLICE_PRELOAD_TORCH", "1") == "1":
        # torch wheels bundle their own libamdhip64 (same soname).  Loading torch first makes this
        # library bind to the SAME HIP runtime, so torch streams/pointers are valid in it.
        try:
            import torch  # noqa: F401
        except Exception:
            pass


def _bind(L, table, strict):
    for name, (res, args) in table.items():
        if not strict and not hasattr(L, name):
            continue
        fn = getattr(L, name)          # AttributeError if the header and the library disagree
        fn.restype = res
        fn.argtypes = args
    return L


# What a build of the library may hold beyond the product: feature -> (its table, the symbol `has_<feature>` keys on, what
# _feature_lib says where it is missing).  The opt-in libraries of _build.LIBRARIES under their names, and the test hooks.
_FEATURES = {
    "hooks": (HOOKS_ABI, "ss_debug_fail_next_scans",
              "this entry point exists in builds with -DSS_TEST_HOOKS only (libsliceslice_hip_tuning.so: "
              "`with ss.tuning_build():` or SLICESLICE_HIP_LIB=<path>)"),
    "service": (SERVICE_ABI, "ss_service_start",
                "the resident search service is not part of libsliceslice_hip.so: it lives in "
                "libsliceslice_hip_service.so (`with ss.service_build():`, or SLICESLICE_HIP_LIB=<path>) "
                "and in the hooks builds"),
    "matches": (MATCHES_ABI, "ss_count_device",
                "count / find_all are not part of libsliceslice_hip.so: they live in "
                "libsliceslice_hip_matches.so - create the searcher inside `with ss.matches_build():`"),
    "matches_batched": (MATCHES_BATCHED_ABI, "ss_count_batched",
                        "count_batched / find_all_batched are not part of this library: they live in "
                        "libsliceslice_hip_matches_batched.so - call them inside `with ss.matches_batched_build():`"),
    "lines": (LINES_ABI, "ss_count_lines_device",
              "count_lines / find_lines are not part of this library: they live in "
              "libsliceslice_hip_lines.so - create the searcher inside `with ss.lines_build():`"),
    "nocase": (NOCASE_ABI, "ss_count_nocase_device",
               "ignore_case=True / new_nocase are not part of this library: they live in "
               "libsliceslice_hip_nocase.so - create the searcher inside `with ss.nocase_build():`"),
    "bounded": (BOUNDED_ABI, "ss_count_bounded_device",
                "whole_word=True / whole_line=True are not part of this library: they live in "
                "libsliceslice_hip_bounded.so - create the searcher inside `with ss.bounded_build():`"),
    "inverted": (INVERTED_ABI, "ss_count_lines_inverted_device",
                 "the inverted line calls (count_lines_inverted / find_lines_inverted, grep -v) are not part of this library: they "
                 "live in libsliceslice_hip_inverted.so - create the searcher inside `with ss.inverted_build():`"),
    "context": (CONTEXT_ABI, "ss_lines_around_device",
                "the context calls (find_lines_context / lines_around, grep -A / -B / -C) are not part of this library: they "
                "live in libsliceslice_hip_context.so - create the searcher inside `with ss.context_build():`"),
    "anyof": (ANYOF_ABI, "ss_union_numbers_device",
              "the several-needle calls (count_lines_anyof / find_lines_anyof / union_numbers, grep -e A -e B) are not part of this "
              "library: they live in libsliceslice_hip_anyof.so - create the searchers inside `with ss.anyof_build():`"),
    "needleset": (NEEDLESET_ABI, "ss_needle_set_new",
                  "the needle-set calls (ss.NeedleSet: count_lines / find_lines for many needles in one pass, grep -f FILE) are not "
                  "part of this library: they live in libsliceslice_hip_needleset.so - create the set inside `with ss.needleset_build():`"),
    "setmatches": (SETMATCHES_ABI, "ss_count_set_device",
                   "the occurrence calls of a needle set (ss.NeedleSet: ranks / count / count_total / count_async / find_all / "
                   "find_all_into) are not part of this library: they live in libsliceslice_hip_setmatches.so - create the set "
                   "inside `with ss.setmatches_build():`"),
    "disjoint": (DISJOINT_ABI, "ss_count_disjoint_device",
                 "the non-overlapping calls (count_disjoint / find_all_disjoint / find_all_disjoint_into / replace / "
                 "select_disjoint / select_disjoint_into) are not part of this library: they live in "
                 "libsliceslice_hip_disjoint.so - create the searcher inside `with ss.disjoint_build():`"),
    "output": (OUTPUT_ABI, "ss_format_lines_device",
               "the output calls (format_lines / format_lines_into / gather_ranges / grep / grep_anyof / NeedleSet.grep) are not part "
               "of this library: they live in libsliceslice_hip_output.so - create the searcher inside `with ss.output_build():`"),
    "leftmost": (LEFTMOST_ABI, "ss_select_leftmost_device",
                 "the leftmost-longest calls (NeedleSet.count_leftmost / find_all_leftmost / find_all_leftmost_into / replace / "
                 "lengths, select_leftmost / select_leftmost_into) are not part of this library: they live in "
                 "libsliceslice_hip_leftmost.so - create the set inside `with ss.leftmost_build():`"),
    "masked": (MASKED_ABI, "ss_masked_new",
               "the masked-pattern calls (ss.MaskedPattern: count / count_async / find_all / find_all_into / count_lines / find_lines / "
               "find_lines_into / info, ss.parse_hex, ss.masked_choose_filter) are not part of this library: they live in "
               "libsliceslice_hip_masked.so - create the pattern inside `with ss.masked_build():`"),
    "classes": (CLASSES_ABI, "ss_classes_new",
                "the byte-class calls (ss.ClassPattern: count / count_async / find_all / find_all_into / count_lines / find_lines / "
                "find_lines_into / info, ss.parse_classes, ss.classes_cover) are not part of this library: they live in "
                "libsliceslice_hip_classes.so - create the pattern inside `with ss.classes_build():`"),
    "runs": (RUNS_ABI, "ss_runs_new",
             "the run calls (ss.RunPattern: count / count_async / find_all / find_all_into / count_lines / find_lines / "
             "find_lines_into / info, ss.parse_runs) are not part of this library: they live in "
             "libsliceslice_hip_runs.so - create the pattern inside `with ss.runs_build():`"),
    "rewrite": (REWRITE_ABI, "ss_replace_runs_device",
                "the rewrite calls (ss.RunPattern: replace / replace_into / delete) are not part of this library: they live in "
                "libsliceslice_hip_rewrite.so - create the pattern inside `with ss.rewrite_build():`"),
    "fields": (FIELDS_ABI, "ss_fields_new",
               "the field calls (ss.FieldSelector: count / find / find_into / cut / info, ss.parse_fields) are not part of this "
               "library: they live in libsliceslice_hip_fields.so - create the selector inside `with ss.fields_build():`"),
    "groups": (GROUPS_ABI, "ss_group_ranges_device",
               "the grouping calls (ss.group_ranges / group_ranges_into / group_lines / groups_scratch_bytes, ss.RunPattern: groups / "
               "most_common) are not part of this library: they live in libsliceslice_hip_groups.so - call them, and create the "
               "pattern, inside `with ss.groups_build():`"),
}


def _load(path):
    """One build of the library: every product symbol must be there; the optional tables are bound where the build has them."""
    _preload_torch()
    L = ctypes.CDLL(path, mode=ctypes.RTLD_LOCAL)
    _bind(L, ABI, strict=True)
    for feature, (table, symbol, _) in _FEATURES.items():
        _bind(L, table, strict=False)
        setattr(L, "has_" + feature, hasattr(L, symbol))
    return L


def _feature_lib(L, feature):
    """`L`, if that build of the library holds `feature` (a key of _FEATURES); else the error that says which build does."""
    if not getattr(L, "has_" + feature, False):
        raise SlicesliceError(SS_ERR_ARGUMENT, _FEATURES[feature][2])
    return L


def lib():
    """Loads csrc/libsliceslice_hip.so (building it with hipcc if it is missing).  Fails loudly.
    SLICESLICE_HIP_LIB=<path> loads another build of the SAME library instead (the tuning build, an A/B build)."""
    global _lib
    if _lib is None:
        _lib = _load(os.environ.get("SLICESLICE_HIP_LIB") or _build.build())
    return _lib


_tools = None
_loaded = {}          # _library_build: name -> the loaded library


def tools_lib():
    """csrc/libsliceslice_hip_tools.so: the benchmark helpers (synthetic haystack generator, read ceiling, self-test)."""
    global _tools
    if _tools is None:
        _build.build()
        _preload_torch()
        _tools = _bind(ctypes.CDLL(_build.tools_library_path(), mode=ctypes.RTLD_LOCAL), TOOLS_ABI, strict=True)
    return _tools


class _library_build:
    """``with ss.<name>_build():`` - inside the block ``lib()`` is libsliceslice_hip_<name>.so (a key of _build.LIBRARIES,
    or "tuning"), built and loaded on first use; blocks nest.  Objects remember the library they were made with, so searchers created
    inside keep working (and are freed by the right library) after the block - and a searcher can only use what ITS library holds.
    The subclasses below say what each library adds."""
    name = None

    def __enter__(self):
        global _lib
        if self.name not in _loaded:
            _loaded[self.name] = _load(_build.build_tuning() if self.name == "tuning" else _build.build_library(self.name))
        self._saved, _lib = _lib, _loaded[self.name]
        return _lib

    def __exit__(self, *a):
        global _lib
        _lib = self._saved
        return False


class tuning_build(_library_build):
    """libsliceslice_hip_tuning.so: every kernel variant and the test hooks of include/sliceslice_hip_tuning.h."""
    name = "tuning"


class service_build(_library_build):
    """libsliceslice_hip_service.so: the product library plus the resident search service (include/sliceslice_hip_service.h).  The
    searchers a SearchService is asked about must be created inside the block too."""
    name = "service"


class matches_build(_library_build):
    """libsliceslice_hip_matches.so: the product library plus the all-matches scan (include/sliceslice_hip_matches.h: ``count`` /
    ``find_all`` of searchers created inside the block)."""
    name = "matches"


class matches_batched_build(_library_build):
    """libsliceslice_hip_matches_batched.so: the matches library plus ``count_batched`` / ``find_all_batched``
    (include/sliceslice_hip_matches_batched.h), which must be called inside the block."""
    name = "matches_batched"


class lines_build(_library_build):
    """libsliceslice_hip_lines.so: the matches library plus the matching-lines scan (include/sliceslice_hip_lines.h: ``count_lines`` /
    ``find_lines`` of searchers created inside the block)."""
    name = "lines"


class nocase_build(_library_build):
    """libsliceslice_hip_nocase.so: the lines library plus the forms ignoring ASCII case (include/sliceslice_hip_nocase.h:
    ``ignore_case=True`` on ``count`` / ``find_all`` / ``count_lines`` / ``find_lines`` of searchers created inside the block, and
    ``DynamicHipSearcher.new_nocase``)."""
    name = "nocase"


class bounded_build(_library_build):
    """libsliceslice_hip_bounded.so: the nocase library plus the whole-word / whole-line forms (include/sliceslice_hip_bounded.h:
    ``whole_word=True`` on ``count`` / ``find_all`` / ``count_lines`` / ``find_lines`` and ``whole_line=True`` on the two line
    methods of searchers created inside the block; both combine with ``ignore_case=True``)."""
    name = "bounded"


class inverted_build(_library_build):
    """libsliceslice_hip_inverted.so: the bounded library plus the lines that do NOT match (include/sliceslice_hip_inverted.h:
    ``count_lines_inverted`` / ``count_lines_inverted_async`` / ``find_lines_inverted`` / ``find_lines_inverted_into`` of searchers
    created inside the block - ``grep -v``; they take ``ignore_case``, ``whole_word`` and ``whole_line`` like their models).  There
    is no inverted ``count`` / ``find_all``: occurrences have no complement."""
    name = "inverted"


class context_build(_library_build):
    """libsliceslice_hip_context.so: the inverted library plus matching lines with their context lines
    (include/sliceslice_hip_context.h: ``find_lines_context`` / ``find_lines_context_into`` - ``grep -A / -B / -C``; they take
    ``ignore_case``, ``whole_word``, ``whole_line`` and ``invert`` - and ``lines_around`` / ``lines_around_into``, the records and the
    context of any ascending set of line numbers, of searchers created inside the block)."""
    name = "context"


class anyof_build(_library_build):
    """libsliceslice_hip_anyof.so: the context library plus the lines that match ANY OF SEVERAL NEEDLES
    (include/sliceslice_hip_anyof.h: ``ss.count_lines_anyof`` / ``ss.find_lines_anyof`` / ``ss.find_lines_anyof_into`` -
    ``grep -e A -e B`` / ``grep -f FILE``; they take ``ignore_case``, ``whole_word``, ``whole_line`` and ``invert``, and the find
    calls ``before`` / ``after`` - of searchers created inside the block, and ``ss.union_numbers`` / ``ss.union_numbers_into``, the
    ordered union of ascending lists of line numbers or its complement)."""
    name = "anyof"


class needleset_build(_library_build):
    """libsliceslice_hip_needleset.so: the anyof library plus the lines that match any of MANY needles, selected in ONE pass over
    the haystack (include/sliceslice_hip_needleset.h: ``ss.NeedleSet(needles, ignore_case=False)`` with ``count_lines`` /
    ``find_lines`` / ``find_lines_into`` / ``info`` - ``grep -e A -e B`` / ``grep -f FILE``; they take ``whole_word``,
    ``whole_line`` and ``invert``, and the find calls ``before`` / ``after`` - of sets created inside the block; every anyof call
    is there beside them for comparison)."""
    name = "needleset"


class setmatches_build(_library_build):
    """libsliceslice_hip_setmatches.so: the needleset library plus every occurrence of every needle of a set in ONE pass over the
    haystack (include/sliceslice_hip_setmatches.h: ``ranks`` / ``count`` / ``count_total`` / ``count_async`` / ``find_all`` /
    ``find_all_into`` of ``ss.NeedleSet`` objects created inside the block - a word-frequency table and the ascending
    (offset, needle) pairs; they take ``whole_word``)."""
    name = "setmatches"


class disjoint_build(_library_build):
    """libsliceslice_hip_disjoint.so: the setmatches library plus the NON-OVERLAPPING occurrences of a needle
    (include/sliceslice_hip_disjoint.h: ``count_disjoint`` / ``find_all_disjoint`` / ``find_all_disjoint_into`` / ``replace`` of
    searchers created inside the block - ``bytes.count``, ``grep -o``, ``bytes.replace``; they take ``ignore_case`` and
    ``whole_word`` - and ``ss.select_disjoint`` / ``ss.select_disjoint_into``, the greedy selection over any ascending list of
    offsets)."""
    name = "disjoint"


class output_build(_library_build):
    """libsliceslice_hip_output.so: the disjoint library plus GREP'S OUTPUT written on the device
    (include/sliceslice_hip_output.h: ``ss.format_lines`` / ``ss.format_lines_into`` - the text of a list of records with line
    numbers, ``:`` / ``-``, terminators and ``--`` separators - ``ss.gather_ranges``, the gather of any list of ranges,
    ``grep`` of searchers created inside the block - ``grep -n -A / -B / -C -F``'s stdout as a device tensor; it takes
    ``ignore_case``, ``whole_word``, ``whole_line`` and ``invert`` - and ``ss.grep_anyof`` / ``NeedleSet.grep``)."""
    name = "output"


class leftmost_build(_library_build):
    """libsliceslice_hip_leftmost.so: the output library plus the LEFTMOST-LONGEST, non-overlapping occurrences of a needle set
    (include/sliceslice_hip_leftmost.h: ``count_leftmost`` / ``find_all_leftmost`` / ``find_all_leftmost_into`` / ``replace`` /
    ``lengths`` of ``ss.NeedleSet`` objects created inside the block - ``grep -o -F -f FILE``, aho_corasick's leftmost-longest
    ``find_iter`` and ``replace_all``, ``re.sub`` over an alternation of literals; they take ``whole_word`` - and
    ``ss.select_leftmost`` / ``ss.select_leftmost_into``, that selection over any list of (offset, length) entries)."""
    name = "leftmost"


class masked_build(_library_build):
    """libsliceslice_hip_masked.so: the leftmost library plus BYTE PATTERNS WITH WILDCARDS AND PER-BYTE MASKS, searched in one pass
    (include/sliceslice_hip_masked.h: ``ss.MaskedPattern(value, mask)`` / ``.from_hex("48 8b ?? 4?")`` /
    ``.from_bytes(b"intel", ignore_case=True)`` with ``count`` / ``count_async`` / ``find_all`` / ``find_all_into`` /
    ``count_lines`` / ``find_lines`` / ``find_lines_into`` / ``info`` of patterns created inside the block, and ``ss.parse_hex`` /
    ``ss.masked_choose_filter``, which are host only)."""
    name = "masked"


class classes_build(_library_build):
    """libsliceslice_hip_classes.so: the masked library plus FIXED-LENGTH PATTERNS OF BYTE CLASSES, searched in one pass
    (include/sliceslice_hip_classes.h: ``ss.ClassPattern(r"[0-9A-F]{4}H")`` / ``.from_sets`` / ``.from_masked`` / ``.from_bytes``
    with ``count`` / ``count_async`` / ``find_all`` / ``find_all_into`` / ``count_lines`` / ``find_lines`` / ``find_lines_into`` /
    ``info`` of patterns created inside the block, and ``ss.parse_classes`` / ``ss.classes_cover``, which are host only)."""
    name = "classes"


class runs_build(_library_build):
    """libsliceslice_hip_runs.so: the classes library plus the MAXIMAL RUNS OF ONE BYTE CLASS, counted and listed in one pass
    (include/sliceslice_hip_runs.h: ``ss.RunPattern(r"[0-9]{3,}")`` / ``.from_set`` with ``count`` / ``count_async`` / ``find_all`` /
    ``find_all_into`` / ``count_lines`` / ``find_lines`` / ``find_lines_into`` / ``info`` of patterns created inside the block, and
    ``ss.parse_runs``, which is host only)."""
    name = "runs"


class rewrite_build(_library_build):
    """libsliceslice_hip_rewrite.so: the runs library plus the SELECTED RUNS REPLACED OR DELETED on the device
    (include/sliceslice_hip_rewrite.h: ``replace`` / ``replace_into`` / ``delete`` of ``ss.RunPattern`` objects created inside the
    block - ``tr -d``, ``tr -s``, ``sed -E 's/[0-9]+/N/g'``; they take a ``delimiter`` that is never a member)."""
    name = "rewrite"


class fields_build(_library_build):
    """libsliceslice_hip_fields.so: the rewrite library plus FIELDS first .. last OF EVERY LINE, located on the device
    (include/sliceslice_hip_fields.h: ``ss.FieldSelector(b",", 3)`` / ``ss.FieldSelector(r"[ \\t]", 2, merge=True)`` with ``count`` /
    ``find`` / ``find_into`` / ``cut`` / ``info`` of selectors created inside the block - ``cut -d, -f3``, ``awk '{print $2}'`` - and
    ``ss.parse_fields``, which is host only)."""
    name = "fields"


class groups_build(_library_build):
    """libsliceslice_hip_groups.so: the fields library plus EQUAL TOKENS OR LINES GROUPED AND COUNTED on the device
    (include/sliceslice_hip_groups.h: ``ss.group_ranges`` / ``ss.group_ranges_into`` over any list of ranges, ``groups`` /
    ``most_common`` of ``ss.RunPattern`` objects created inside the block - ``grep -oE '\\w+' | sort | uniq -c`` - ``ss.group_lines`` -
    ``sort | uniq -c``, ``awk '!seen[$0]++'`` - and ``ss.groups_scratch_bytes``, which is host only)."""
    name = "groups"


_FOLD_TABLE = bytes(b | 0x20 if 0x41 <= b <= 0x5A else b for b in range(256))


def fold_ascii(data):
    """``data`` with the bytes 'A'..'Z' replaced by 'a'..'z' and every other byte value as it is - the fold of the calls that
    ignore ASCII case (``bytes.lower()``)."""
    return bytes(data).translate(_FOLD_TABLE)


def is_word_byte(b):
    """True for the word bytes of the whole-word forms (include/sliceslice_hip_bounded.h): '0'..'9', 'A'..'Z', 'a'..'z' and '_' -
    ``grep -w`` in the C locale.  No byte >= 0x80 is one."""
    b = int(b)
    return 0x30 <= b <= 0x39 or 0x41 <= b <= 0x5A or 0x61 <= b <= 0x7A or b == 0x5F


def _delimiter_byte(delimiter):
    """The one delimiter byte of count_lines / find_lines: an int 0..255 or a bytes object of length one."""
    if isinstance(delimiter, (bytes, bytearray)):
        if len(delimiter) != 1:
            raise ValueError("the line delimiter is ONE byte, got %d" % len(delimiter))
        return delimiter[0]
    return int(delimiter)


def _scan_fn(L, name, ignore_case, whole_word=False, whole_line=False, invert=False):
    """The function `name` of the matches or the lines library from `L`, or - ignore_case - its folding form from the nocase
    library: ss_count_device -> ss_count_nocase_device, ss_find_lines_device -> ss_find_lines_nocase_device, ...
    whole_word / whole_line: its form in the bounded library (ss_count_bounded_device, ...) behind the SAME argument list - `how`
    (SS_BOUND_WORD / SS_BOUND_LINE, | SS_BOUND_NOCASE with ignore_case) goes in front of the stream here.
    invert (line functions only): the form in the inverted library (ss_count_lines_inverted_device, ...), whose `how` may also be 0
    or SS_BOUND_NOCASE alone."""
    if invert or whole_word or whole_line:
        fn = getattr(_feature_lib(L, "inverted"), name.replace("_device", "_inverted_device")) if invert else \
            getattr(_feature_lib(L, "bounded"), name.replace("_device", "_bounded_device"))
        how = (SS_BOUND_WORD if whole_word else 0) | (SS_BOUND_LINE if whole_line else 0) | (SS_BOUND_NOCASE if ignore_case else 0)
        at = 4 if "_lines_" in name else 3                  # (searcher, haystack, len[, delimiter], HOW, stream, ...)
        return lambda *a: fn(*a[:at], how, *a[at:])
    if ignore_case:
        return getattr(_feature_lib(L, "nocase"), name.replace("_device", "_nocase_device"))
    return getattr(_feature_lib(L, "lines" if "_lines_" in name else "matches"), name)


def _check(rc, L=None):
    if rc != SS_OK:
        msg = (L or lib()).ss_last_error().decode("utf-8", "replace")
        raise (PositionError if rc == SS_ERR_POSITION else SlicesliceError)(rc, msg)


def _check_tools(rc):
    if rc != SS_OK:
        raise SlicesliceError(rc, tools_lib().ss_tools_last_error().decode("utf-8", "replace"))


def _host_view(b):
    """(keepalive, address, length) of a host buffer."""
    if isinstance(b, np.ndarray):
        a = np.ascontiguousarray(b, dtype=np.uint8)
        return a, (a.ctypes.data if a.size else 0), a.size
    if isinstance(b, bytes):
        a = np.frombuffer(b, dtype=np.uint8)
        return (a, b), (a.ctypes.data if a.size else 0), a.size
    if isinstance(b, (bytearray, memoryview)):
        a = np.frombuffer(b, dtype=np.uint8)
        return (a, b), (a.ctypes.data if a.size else 0), a.size
    raise TypeError("unsupported haystack/needle type %r" % type(b))


def _is_tensor(x):
    return type(x).__module__.split(".")[0] == "torch" and hasattr(x, "data_ptr")


def _current_stream_handle():
    if "torch" in sys.modules:
        import torch
        if torch.cuda.is_available():
            return torch.cuda.current_stream().cuda_stream
    return 0


class _on_device_of:
    """The C side launches on the CURRENT device (its needle copy, its flag slots) and, by default, on torch's
    current stream OF THAT DEVICE: make the tensor's device current for the duration of the call, so that a
    haystack on cuda:1 is never scanned by a kernel launched on cuda:0."""

    def __init__(self, t):
        self._ctx = None
        if _is_tensor(t) and t.is_cuda:
            import torch
            if t.device.index != torch.cuda.current_device():
                self._ctx = torch.cuda.device(t.device)

    def __enter__(self):
        if self._ctx is not None:
            self._ctx.__enter__()
        return self

    def __exit__(self, *a):
        if self._ctx is not None:
            self._ctx.__exit__(*a)
        return False


# The four line methods of DynamicHipSearcher and their inverted twins (`invert`: the lines that do NOT match).  Functions of
# the module, so that a call fails on the library's refusal before it touches anything else of the searcher.
def _count_lines(s, invert, haystack, delimiter=b"\n", stream=None, ignore_case=False, whole_word=False, whole_line=False):
    fn = _scan_fn(s._L, "ss_count_lines_device", ignore_case, whole_word, whole_line, invert)
    ptr, length, t = s._device_haystack(haystack)
    c = _u64(0)
    with _on_device_of(t):
        st = stream if stream is not None else _current_stream_handle()
        s._ck(fn(s._h, ptr, length, _delimiter_byte(delimiter), st, ctypes.byref(c)))
    return c.value


def _count_lines_async(s, invert, haystack, d_count, delimiter=b"\n", stream=None, ignore_case=False, whole_word=False, whole_line=False):
    fn = _scan_fn(s._L, "ss_count_lines_device_async", ignore_case, whole_word, whole_line, invert)
    with _on_device_of(haystack):
        st = stream if stream is not None else _current_stream_handle()
        s._ck(fn(s._h, haystack.data_ptr(), haystack.numel(), _delimiter_byte(delimiter), st, d_count.data_ptr()))


def _find_lines(s, invert, haystack, delimiter=b"\n", capacity=None, stream=None, ignore_case=False, whole_word=False, whole_line=False):
    import torch
    count_fn, find_fn = _scan_fn(s._L, "ss_count_lines_device", ignore_case, whole_word, whole_line, invert), _scan_fn(s._L, "ss_find_lines_device", ignore_case, whole_word, whole_line, invert)
    ptr, length, t = s._device_haystack(haystack)
    dev = t.device if t is not None else torch.device("cuda", torch.cuda.current_device())
    d = _delimiter_byte(delimiter)
    total = _u64(0)
    with _on_device_of(t):
        st = stream if stream is not None else _current_stream_handle()
        if capacity is None:
            s._ck(count_fn(s._h, ptr, length, d, st, ctypes.byref(total)))
            capacity = total.value
        out = torch.empty((3, max(int(capacity), 1)), dtype=torch.int64, device=dev)
        p = [out[k].data_ptr() if capacity else None for k in range(3)]
        s._ck(find_fn(s._h, ptr, length, d, st, p[0], p[1], p[2], int(capacity), ctypes.byref(total)))
    k = min(int(capacity), total.value)
    return out[0, :k], out[1, :k], out[2, :k]


def _find_lines_into(s, invert, haystack, d_begin, d_end, d_number, capacity, delimiter=b"\n", stream=None, ignore_case=False, whole_word=False, whole_line=False):
    fn = _scan_fn(s._L, "ss_find_lines_device", ignore_case, whole_word, whole_line, invert)
    ptr, length, t = s._device_haystack(haystack)
    total = _u64(0)
    with _on_device_of(t):
        st = stream if stream is not None else _current_stream_handle()
        p = [x.data_ptr() if x is not None else None for x in (d_begin, d_end, d_number)]
        s._ck(fn(s._h, ptr, length, _delimiter_byte(delimiter), st, p[0], p[1], p[2], int(capacity), ctypes.byref(total)))
    return total.value


# The four context methods of DynamicHipSearcher (include/sliceslice_hip_context.h), functions of the module for the same reason.
_U64_MAX = (1 << 64) - 1


def _context_amount(value, what):
    value = int(value)
    if not 0 <= value <= _U64_MAX:
        raise ValueError("%s is a number of lines, 0 .. 2^64 - 1, got %d" % (what, value))
    return value


def _context_how(ignore_case, whole_word, whole_line, invert):
    return (SS_BOUND_WORD if whole_word else 0) | (SS_BOUND_LINE if whole_line else 0) | (SS_BOUND_NOCASE if ignore_case else 0) | \
        (SS_CONTEXT_INVERT if invert else 0)


def _device_numbers(numbers, dev):
    """The line numbers of lines_around as an int64 device tensor (a tensor on the device is taken as it is)."""
    import torch
    if _is_tensor(numbers):
        if numbers.dtype not in (torch.int64, torch.uint64):
            raise TypeError("line numbers are 64-bit integers")
        return numbers.contiguous().to(dev)
    a = np.ascontiguousarray(np.asarray(numbers, dtype=np.uint64)).view(np.int64).reshape(-1)
    return torch.from_numpy(a.copy()).to(dev)


def _context_arrays(capacity, dev):
    import torch
    n = max(int(capacity), 1)
    return torch.empty((3, n), dtype=torch.int64, device=dev), torch.empty(n, dtype=torch.uint8, device=dev)


def _find_lines_context_into(s, haystack, d_begin, d_end, d_number, d_kind, capacity, before=0, after=0, delimiter=b"\n", stream=None,
                             ignore_case=False, whole_word=False, whole_line=False, invert=False):
    fn = _feature_lib(s._L, "context").ss_find_lines_context_device
    ptr, length, t = s._device_haystack(haystack)
    total, selected = _u64(0), _u64(0)
    with _on_device_of(t):
        st = stream if stream is not None else _current_stream_handle()
        p = [x.data_ptr() if x is not None else None for x in (d_begin, d_end, d_number, d_kind)]
        s._ck(fn(s._h, ptr, length, _delimiter_byte(delimiter), _context_how(ignore_case, whole_word, whole_line, invert),
                 _context_amount(before, "before"), _context_amount(after, "after"), st, p[0], p[1], p[2], p[3], int(capacity),
                 ctypes.byref(total), ctypes.byref(selected)))
    return total.value, selected.value


def _find_lines_context(s, haystack, before=0, after=0, delimiter=b"\n", capacity=None, stream=None, ignore_case=False, whole_word=False,
                        whole_line=False, invert=False):
    import torch
    _feature_lib(s._L, "context")
    ptr, length, t = s._device_haystack(haystack)
    dev = t.device if t is not None else torch.device("cuda", torch.cuda.current_device())
    kw = dict(before=before, after=after, delimiter=delimiter, stream=stream, ignore_case=ignore_case, whole_word=whole_word,
              whole_line=whole_line, invert=invert)
    hay = t if t is not None else (ptr, length)
    if capacity is None:
        capacity, _ = _find_lines_context_into(s, hay, None, None, None, None, 0, **kw)
    out, kind = _context_arrays(capacity, dev)
    p = [out[k] if capacity else None for k in range(3)] + [kind if capacity else None]
    total, _ = _find_lines_context_into(s, hay, p[0], p[1], p[2], p[3], capacity, **kw)
    k = min(int(capacity), total)
    return out[0, :k], out[1, :k], out[2, :k], kind[:k]


def _lines_around_into(s, haystack, numbers, d_begin, d_end, d_number, d_kind, capacity, before=0, after=0, delimiter=b"\n", stream=None):
    import torch
    fn = _feature_lib(s._L, "context").ss_lines_around_device
    ptr, length, t = s._device_haystack(haystack)
    dev = t.device if t is not None else torch.device("cuda", torch.cuda.current_device())
    total = _u64(0)
    with _on_device_of(t):
        d_numbers = _device_numbers(numbers, dev)
        st = stream if stream is not None else _current_stream_handle()
        p = [x.data_ptr() if x is not None else None for x in (d_begin, d_end, d_number, d_kind)]
        s._ck(fn(s._h, ptr, length, _delimiter_byte(delimiter), d_numbers.data_ptr() if d_numbers.numel() else None, d_numbers.numel(),
                 _context_amount(before, "before"), _context_amount(after, "after"), st, p[0], p[1], p[2], p[3], int(capacity),
                 ctypes.byref(total)))
    return total.value


def _lines_around(s, haystack, numbers, before=0, after=0, delimiter=b"\n", capacity=None, stream=None):
    import torch
    _feature_lib(s._L, "context")
    ptr, length, t = s._device_haystack(haystack)
    dev = t.device if t is not None else torch.device("cuda", torch.cuda.current_device())
    hay = t if t is not None else (ptr, length)
    with _on_device_of(t):
        numbers = _device_numbers(numbers, dev)
    kw = dict(before=before, after=after, delimiter=delimiter, stream=stream)
    if capacity is None:
        capacity = _lines_around_into(s, hay, numbers, None, None, None, None, 0, **kw)
    out, kind = _context_arrays(capacity, dev)
    p = [out[k] if capacity else None for k in range(3)] + [kind if capacity else None]
    total = _lines_around_into(s, hay, numbers, p[0], p[1], p[2], p[3], capacity, **kw)
    k = min(int(capacity), total)
    return out[0, :k], out[1, :k], out[2, :k], kind[:k]


def lines_around(haystack, numbers, before=0, after=0, delimiter=b"\n", capacity=None, stream=None):
    """``DynamicHipSearcher.lines_around`` through a throw-away searcher (the call needs one for the device and its scratch only;
    inside ``with ss.context_build():``)."""
    return DynamicHipSearcher.new(b"").lines_around(haystack, numbers, before, after, delimiter, capacity, stream)


# The several-needle calls (include/sliceslice_hip_anyof.h): functions of the module, since no searcher owns them.
def _anyof_table(searchers):
    """(the library, the table of handles, its length) of a non-empty sequence of searchers made inside ``with ss.anyof_build():``."""
    inner = [getattr(s, "_inner", s) for s in searchers]
    L = _feature_lib(inner[0]._L if inner else lib(), "anyof")
    if not inner:
        raise SlicesliceError(SS_ERR_ARGUMENT, "the several-needle calls take at least one searcher")
    if any(s._L is not L for s in inner):
        raise SlicesliceError(SS_ERR_ARGUMENT, "the searchers of a several-needle call belong to one library: create all of them inside "
                                               "one `with ss.anyof_build():`")
    return L, inner, (ctypes.c_void_p * len(inner))(*[s._h for s in inner])


def count_lines_anyof(searchers, haystack, delimiter=b"\n", stream=None, ignore_case=False, whole_word=False, whole_line=False, invert=False):
    """The number of lines that hold ANY of the searchers' needles - ``grep -c -e A -e B`` (ss_count_lines_anyof_device); with
    ``invert`` the lines that hold none of them.  The flags apply to every needle."""
    L, inner, table = _anyof_table(searchers)
    ptr, length, t = inner[0]._device_haystack(haystack)
    c = _u64(0)
    with _on_device_of(t):
        st = stream if stream is not None else _current_stream_handle()
        _check(L.ss_count_lines_anyof_device(table, len(inner), ptr, length, _delimiter_byte(delimiter),
                                             _context_how(ignore_case, whole_word, whole_line, invert), st, ctypes.byref(c)), L)
    return c.value


def find_lines_anyof_into(searchers, haystack, d_begin, d_end, d_number, d_kind, capacity, before=0, after=0, delimiter=b"\n", stream=None,
                          ignore_case=False, whole_word=False, whole_line=False, invert=False):
    """ss_find_lines_anyof_device into the caller's device tensors (8-byte x3, 1-byte kind; each may be None); returns
    (total, selected)."""
    L, inner, table = _anyof_table(searchers)
    ptr, length, t = inner[0]._device_haystack(haystack)
    total, selected = _u64(0), _u64(0)
    with _on_device_of(t):
        st = stream if stream is not None else _current_stream_handle()
        p = [x.data_ptr() if x is not None else None for x in (d_begin, d_end, d_number, d_kind)]
        _check(L.ss_find_lines_anyof_device(table, len(inner), ptr, length, _delimiter_byte(delimiter),
                                            _context_how(ignore_case, whole_word, whole_line, invert), _context_amount(before, "before"),
                                            _context_amount(after, "after"), st, p[0], p[1], p[2], p[3], int(capacity), ctypes.byref(total),
                                            ctypes.byref(selected)), L)
    return total.value, selected.value


def find_lines_anyof(searchers, haystack, before=0, after=0, delimiter=b"\n", capacity=None, stream=None, ignore_case=False, whole_word=False,
                     whole_line=False, invert=False):
    """(begin, end, number, kind) of the lines that hold ANY of the searchers' needles, with ``before`` lines in front of and
    ``after`` lines behind each of them, every line once, ascending - ``grep -n -e A -e B`` with ``-B`` / ``-A``
    (ss_find_lines_anyof_device); kind is 1 for a selected line and 0 for a context line."""
    import torch
    L, inner, table = _anyof_table(searchers)
    ptr, length, t = inner[0]._device_haystack(haystack)
    dev = t.device if t is not None else torch.device("cuda", torch.cuda.current_device())
    kw = dict(before=before, after=after, delimiter=delimiter, stream=stream, ignore_case=ignore_case, whole_word=whole_word,
              whole_line=whole_line, invert=invert)
    hay = t if t is not None else (ptr, length)
    if capacity is None:
        capacity, _ = find_lines_anyof_into(searchers, hay, None, None, None, None, 0, **kw)
    out, kind = _context_arrays(capacity, dev)
    p = [out[k] if capacity else None for k in range(3)] + [kind if capacity else None]
    total, _ = find_lines_anyof_into(searchers, hay, p[0], p[1], p[2], p[3], capacity, **kw)
    k = min(int(capacity), total)
    return out[0, :k], out[1, :k], out[2, :k], kind[:k]


_UNION_SEARCHERS = {}            # library -> the searcher that union_numbers hands to ss_union_numbers_device


def _union_lists(lists, dev):
    """(the lists' numbers in one int64 device tensor, their CSR offsets as a ctypes array, their number)"""
    import torch
    parts = [_device_numbers(l, dev).reshape(-1) for l in lists]
    offsets = [0]
    for q in parts:
        offsets.append(offsets[-1] + q.numel())
    flat = torch.cat(parts) if parts else torch.empty(0, dtype=torch.int64, device=dev)
    return flat, (ctypes.c_uint64 * len(offsets))(*offsets), len(parts)


def union_numbers_into(lists, limit, d_out, capacity, complement=False, stream=None):
    """ss_union_numbers_device into the caller's 8-byte device tensor (None: count only); returns the size of the union.  Inside
    ``with ss.anyof_build():``."""
    import torch
    L = _feature_lib(lib(), "anyof")
    dev = d_out.device if d_out is not None else next((l.device for l in lists if _is_tensor(l) and l.is_cuda), torch.device("cuda", torch.cuda.current_device()))
    s = _UNION_SEARCHERS.get(id(L)) or _UNION_SEARCHERS.setdefault(id(L), DynamicHipSearcher.new(b""))     # (the call needs one for
                                                                                                           # the device and its scratch only)
    total = _u64(0)
    with _on_device_of(d_out):
        flat, offsets, n = _union_lists(lists, dev)
        st = stream if stream is not None else _current_stream_handle()
        _check(L.ss_union_numbers_device(s._h, flat.data_ptr() if flat.numel() else None, offsets, n, int(limit), 1 if complement else 0, st,
                                         d_out.data_ptr() if d_out is not None else None, int(capacity), ctypes.byref(total)), L)
    return total.value


def union_numbers(lists, limit, complement=False, capacity=None, stream=None):
    """The ascending union of the strictly ascending ``lists`` of line numbers (sequences, arrays or device tensors), each value
    once - or with ``complement`` every number of 1 .. limit that is in no list - as an int64 device tensor of
    min(total, capacity) numbers (ss_union_numbers_device).  A 0 and a number above ``limit`` select nothing.  Inside
    ``with ss.anyof_build():``."""
    import torch
    _feature_lib(lib(), "anyof")
    lists = list(lists)
    dev = next((l.device for l in lists if _is_tensor(l) and l.is_cuda), torch.device("cuda", torch.cuda.current_device()))
    lists = [_device_numbers(l, dev) for l in lists]
    if capacity is None:
        capacity = union_numbers_into(lists, limit, None, 0, complement, stream)
    out = torch.empty(max(int(capacity), 1), dtype=torch.int64, device=dev)
    total = union_numbers_into(lists, limit, out if capacity else None, capacity, complement, stream)
    return out[:min(int(capacity), total)]


def select_disjoint_into(offsets, n, d_out, stream=None):
    """ss_select_disjoint_device into the caller's 8-byte device tensor (capacity = its length; None: count only); returns the size
    of the selection.  Inside ``with ss.disjoint_build():``."""
    import torch
    L = _feature_lib(lib(), "disjoint")
    dev = offsets.device if _is_tensor(offsets) and offsets.is_cuda else (d_out.device if d_out is not None else torch.device("cuda", torch.cuda.current_device()))
    s = _UNION_SEARCHERS.get(id(L)) or _UNION_SEARCHERS.setdefault(id(L), DynamicHipSearcher.new(b""))     # (for the device and its scratch only)
    total = _u64(0)
    with _on_device_of(d_out if d_out is not None else offsets):
        flat = _device_numbers(offsets, dev).reshape(-1)
        st = stream if stream is not None else _current_stream_handle()
        _check(L.ss_select_disjoint_device(s._h, flat.data_ptr() if flat.numel() else None, flat.numel(), int(n), st,
                                           d_out.data_ptr() if d_out is not None and d_out.numel() else None,
                                           d_out.numel() if d_out is not None else 0, ctypes.byref(total)), L)
    return total.value


def select_disjoint(offsets, n, capacity=None, stream=None):
    """The greedy non-overlapping selection over the strictly ascending ``offsets`` (a sequence, an array or a device tensor) of
    occurrences of length ``n``: the first is selected, and after a selected p the first at or beyond p + n - as an int64 device
    tensor of min(total, capacity) offsets (ss_select_disjoint_device).  Inside ``with ss.disjoint_build():``."""
    import torch
    _feature_lib(lib(), "disjoint")
    dev = offsets.device if _is_tensor(offsets) and offsets.is_cuda else torch.device("cuda", torch.cuda.current_device())
    flat = _device_numbers(offsets, dev).reshape(-1)
    if capacity is None:
        capacity = select_disjoint_into(flat, n, None, stream)
    out = torch.empty(max(int(capacity), 1), dtype=torch.int64, device=dev)
    total = select_disjoint_into(flat, n, out[:int(capacity)] if capacity else None, stream)
    return out[:min(int(capacity), total)]


_SCRATCH_SETS = {}


def _scratch_set(L):
    """The needle set of library `L` that ss_select_leftmost_device is handed for the device and its scratch only."""
    global _lib
    s = _SCRATCH_SETS.get(id(L))
    if s is None:
        saved, _lib = _lib, L
        try:
            s = _SCRATCH_SETS.setdefault(id(L), NeedleSet([b"a"]))
        finally:
            _lib = saved
    return s


def select_leftmost_into(offsets, lengths, d_selected, d_which, capacity=None, stream=None):
    """ss_select_leftmost_device into the caller's 8-byte device tensors (each may be None; capacity: default the shorter of
    them, 0 where both are None); returns the size of the selection.  Inside ``with ss.leftmost_build():``."""
    import torch
    L = _feature_lib(lib(), "leftmost")
    given = [x for x in (d_selected, d_which) if x is not None]
    dev = offsets.device if _is_tensor(offsets) and offsets.is_cuda else (given[0].device if given else torch.device("cuda", torch.cuda.current_device()))
    if capacity is None:
        capacity = min(x.numel() for x in given) if given else 0
    total = _u64(0)
    with _on_device_of(given[0] if given else offsets):
        flat = _device_numbers(offsets, dev).reshape(-1)
        lens = _device_numbers(lengths, dev).reshape(-1)
        if lens.numel() != flat.numel():
            raise ValueError("%d offsets and %d lengths" % (flat.numel(), lens.numel()))
        s = _scratch_set(L)
        st = stream if stream is not None else _current_stream_handle()
        _check(L.ss_select_leftmost_device(s._h, flat.data_ptr() if flat.numel() else None, lens.data_ptr() if lens.numel() else None,
                                           flat.numel(), st, d_selected.data_ptr() if d_selected is not None and d_selected.numel() else None,
                                           d_which.data_ptr() if d_which is not None and d_which.numel() else None, int(capacity),
                                           ctypes.byref(total)), L)
    return total.value


def select_leftmost(offsets, lengths, capacity=None, stream=None):
    """The leftmost-longest selection over entries (offsets[j], lengths[j]) - sequences, arrays or device tensors; the offsets
    ascend and may repeat, the lengths ascend within a run of equal offsets: the last entry of a run is its candidate, the first
    candidate is selected, and after a selected p of length l the first candidate at or beyond p + l.  Returns
    (selected offsets, their indices in the list) as int64 device tensors of min(total, capacity) entries
    (ss_select_leftmost_device).  Inside ``with ss.leftmost_build():``."""
    import torch
    _feature_lib(lib(), "leftmost")
    dev = offsets.device if _is_tensor(offsets) and offsets.is_cuda else torch.device("cuda", torch.cuda.current_device())
    flat, lens = _device_numbers(offsets, dev).reshape(-1), _device_numbers(lengths, dev).reshape(-1)
    if capacity is None:
        capacity = select_leftmost_into(flat, lens, None, None, 0, stream)
    out = torch.empty((2, max(int(capacity), 1)), dtype=torch.int64, device=dev)
    total = select_leftmost_into(flat, lens, out[0] if capacity else None, out[1] if capacity else None, int(capacity), stream)
    k = min(int(capacity), total)
    return out[0, :k], out[1, :k]


# The output calls (include/sliceslice_hip_output.h): functions of the module, since no searcher owns them.
def _scratch_searcher(L):
    """The searcher of library `L` that a call which needs one for the device and its scratch only is handed."""
    global _lib
    s = _UNION_SEARCHERS.get(id(L))
    if s is None:
        saved, _lib = _lib, L
        try:
            s = _UNION_SEARCHERS.setdefault(id(L), DynamicHipSearcher.new(b""))
        finally:
            _lib = saved
    return s


def _terminator_byte(terminator):
    """The terminator of the output calls: None (-1, none) or one byte as ``_delimiter_byte`` takes it."""
    return -1 if terminator is None else _delimiter_byte(terminator)


def _device_kinds(kind, dev):
    """The kinds of format_lines as a uint8 device tensor (a 1-byte tensor on the device is taken as it is)."""
    import torch
    if _is_tensor(kind):
        if kind.dtype.itemsize != 1:
            raise TypeError("kinds are 1-byte integers")
        return kind.contiguous().to(dev).view(torch.uint8).reshape(-1)
    return torch.from_numpy(np.ascontiguousarray(np.asarray(kind, dtype=np.uint8)).reshape(-1).copy()).to(dev)


def _output_flags(number, line_numbers, separators):
    return (SS_OUTPUT_NUMBER if (number is not None if line_numbers is None else line_numbers) else 0) | (SS_OUTPUT_SEPARATOR if separators else 0)


def _format_into(L, haystack, begin, end, number, kind, terminator, flags, d_out, d_starts, stream, gather=False):
    """One ss_format_lines_device (gather: ss_gather_ranges_device) call of library `L`; returns *out_len."""
    import torch
    L = _feature_lib(L, "output")
    ptr, length, t = DynamicHipSearcher._device_haystack(haystack)
    dev = t.device if t is not None else next((x.device for x in (begin, d_out) if _is_tensor(x) and x.is_cuda), torch.device("cuda", torch.cuda.current_device()))
    s = _scratch_searcher(L)
    out_len = _u64(0)
    with _on_device_of(t if t is not None else d_out):
        b, e = _device_numbers(begin, dev).reshape(-1), _device_numbers(end, dev).reshape(-1)
        n = _device_numbers(number, dev).reshape(-1) if number is not None else None
        k = _device_kinds(kind, dev) if kind is not None else None
        if any(x is not None and x.numel() != b.numel() for x in (e, n, k)):
            raise ValueError("begin, end, number and kind hold one entry per record")
        if d_starts is not None and d_starts.numel() < b.numel() + 1:
            raise ValueError("d_starts holds count + 1 entries")
        st = stream if stream is not None else _current_stream_handle()
        p = [x.data_ptr() if x is not None and x.numel() else None for x in (b, e, n, k, d_out, d_starts)]
        capacity = d_out.numel() if d_out is not None else 0
        if gather:
            _check(L.ss_gather_ranges_device(s._h, ptr, length, p[0], p[1], b.numel(), _terminator_byte(terminator), st, p[4], capacity, p[5],
                                             ctypes.byref(out_len)), L)
        else:
            _check(L.ss_format_lines_device(s._h, ptr, length, p[0], p[1], p[2], p[3], b.numel(), _terminator_byte(terminator), int(flags), st,
                                            p[4], capacity, p[5], ctypes.byref(out_len)), L)
    return out_len.value


def _format(L, haystack, begin, end, number, kind, terminator, flags, stream, gather=False, return_starts=False):
    """The count-only call, then the sized one: the output as a uint8 device tensor (return_starts: and the count + 1 starts)."""
    import torch
    _feature_lib(L, "output")
    ptr, length, t = DynamicHipSearcher._device_haystack(haystack)
    dev = t.device if t is not None else (begin.device if _is_tensor(begin) and begin.is_cuda else torch.device("cuda", torch.cuda.current_device()))
    hay = t if t is not None else (ptr, length)
    begin, end = _device_numbers(begin, dev).reshape(-1), _device_numbers(end, dev).reshape(-1)
    number = _device_numbers(number, dev).reshape(-1) if number is not None else None
    kind = _device_kinds(kind, dev) if kind is not None else None
    starts = torch.empty(begin.numel() + 1, dtype=torch.int64, device=dev) if return_starts else None
    total = _format_into(L, hay, begin, end, number, kind, terminator, flags, None, starts, stream, gather)
    out = torch.empty(max(total, 1), dtype=torch.uint8, device=dev)
    if total:
        _format_into(L, hay, begin, end, number, kind, terminator, flags, out[:total], None, stream, gather)
    return (out[:total], starts) if return_starts else out[:total]


def format_lines_into(haystack, begin, end, d_out, number=None, kind=None, delimiter=b"\n", line_numbers=None, separators=False, d_starts=None,
                      stream=None):
    """ss_format_lines_device into the caller's 1-byte device tensor ``d_out`` (capacity = its length; None: the length only) and,
    where given, the count + 1 starts into the 8-byte device tensor ``d_starts``; returns the length of the output.  A ``d_out``
    that is too short is left untouched.  Arguments as ``format_lines``.  Inside ``with ss.output_build():``."""
    return _format_into(lib(), haystack, begin, end, number, kind, delimiter, _output_flags(number, line_numbers, separators), d_out, d_starts, stream)


def format_lines(haystack, begin, end, number=None, kind=None, delimiter=b"\n", line_numbers=None, separators=False, stream=None):
    """The text of the records (begin, end, number, kind) of ``haystack`` - what the line calls return; sequences, arrays or device
    tensors - as one uint8 device tensor: for every record ``--`` and the delimiter where ``separators`` is set and its number lies
    more than 1 above the one before, its number and ``:`` (kind != 0, or no kind) or ``-`` where ``line_numbers`` is set (None: set
    exactly when numbers are given), the bytes [begin, end) clamped to the haystack, and the delimiter (None: none) -
    ``grep -n -A / -B / -C``'s stdout (ss_format_lines_device: counted first, then sized exactly).  Any list is formatted: records
    may overlap, repeat or descend.  Inside ``with ss.output_build():``."""
    return _format(lib(), haystack, begin, end, number, kind, delimiter, _output_flags(number, line_numbers, separators), stream)


def gather_ranges(haystack, begin, end, terminator=None, return_starts=False, stream=None):
    """The bytes [begin[i], end[i]) of ``haystack``, clamped to it, one range after the other and each followed by ``terminator``
    (one byte; None: none), as one uint8 device tensor (ss_gather_ranges_device) - what ``grep -o`` and ``sed -n 'Np'`` print from
    a list of ranges.  return_starts: also the int64 device tensor of the count + 1 output offsets at which the ranges begin, the
    last of them the length.  Inside ``with ss.output_build():``."""
    return _format(lib(), haystack, begin, end, None, None, terminator, 0, stream, gather=True, return_starts=return_starts)


def grep_anyof(searchers, haystack, before=0, after=0, delimiter=b"\n", line_numbers=False, stream=None, ignore_case=False, whole_word=False,
               whole_line=False, invert=False):
    """``grep -e A -e B`` 's stdout as a uint8 device tensor: ``find_lines_anyof`` followed by ``format_lines`` (separators exactly
    when ``before`` or ``after`` is non-zero, as in grep).  Searchers made inside ``with ss.output_build():``."""
    searchers = list(searchers)
    L = _feature_lib(getattr(searchers[0], "_inner", searchers[0])._L if searchers else lib(), "output")
    begin, end, number, kind = find_lines_anyof(searchers, haystack, before, after, delimiter, None, stream, ignore_case, whole_word, whole_line,
                                                invert)
    return _format(L, haystack, begin, end, number, kind, delimiter, _output_flags(number, line_numbers, bool(before or after)), stream)


class NeedleSet:
    """A compiled set of needles (ss_needle_set_new, inside ``with ss.needleset_build():``) on the current device.  Its line calls
    select what ``ss.count_lines_anyof`` / ``ss.find_lines_anyof`` select for searchers of the same needles, in one pass over
    the haystack instead of one per needle.  ``ignore_case`` is a property of the set: the needles are folded once, here."""

    def __init__(self, needles, ignore_case=False):
        self._h = None
        self._L = L = _feature_lib(lib(), "needleset")
        views = [_host_view(n.astype(np.uint8).tobytes() if isinstance(n, np.ndarray) else bytes(n)) for n in needles]
        count = len(views)
        table = (ctypes.c_void_p * max(count, 1))(*[v[1] if v[2] else None for v in views])
        lens = (ctypes.c_size_t * max(count, 1))(*[v[2] for v in views])
        h = ctypes.c_void_p()
        _check(L.ss_needle_set_new(table, lens, count, SS_SET_NOCASE if ignore_case else 0, ctypes.byref(h)), L)
        self._h = h
        self._count = count
        self._needles = [bytes(ctypes.string_at(v[1], v[2])) if v[2] else b"" for v in views]      # (for ``replace`` with a mapping)
        self.ignore_case = bool(ignore_case)

    def _how(self, whole_word, whole_line, invert):
        return _context_how(self.ignore_case, whole_word, whole_line, invert)

    def info(self):
        """dict of ss_needle_set_info: needles, distinct, blob_bytes, one_byte, two_byte, prefix_keys, largest_bucket, fold."""
        words = (ctypes.c_uint64 * len(NEEDLESET_STATS))()
        _check(self._L.ss_needle_set_info(self._h, words), self._L)
        return dict(zip(NEEDLESET_STATS, (int(w) for w in words)))

    def count_lines(self, haystack, delimiter=b"\n", whole_word=False, whole_line=False, invert=False, stream=None):
        """The number of lines that hold ANY needle of the set (ss_count_lines_set_device); ``invert``: that hold none."""
        ptr, length, t = DynamicHipSearcher._device_haystack(haystack)
        c = _u64(0)
        with _on_device_of(t):
            st = stream if stream is not None else _current_stream_handle()
            _check(self._L.ss_count_lines_set_device(self._h, ptr, length, _delimiter_byte(delimiter), self._how(whole_word, whole_line, invert),
                                                     st, ctypes.byref(c)), self._L)
        return c.value

    def find_lines_into(self, haystack, d_begin, d_end, d_number, d_kind, capacity, before=0, after=0, delimiter=b"\n", whole_word=False,
                        whole_line=False, invert=False, stream=None):
        """ss_find_lines_set_device into the caller's device tensors (8-byte x3, 1-byte kind; each may be None); returns
        (total, selected)."""
        ptr, length, t = DynamicHipSearcher._device_haystack(haystack)
        total, selected = _u64(0), _u64(0)
        with _on_device_of(t):
            st = stream if stream is not None else _current_stream_handle()
            p = [x.data_ptr() if x is not None else None for x in (d_begin, d_end, d_number, d_kind)]
            _check(self._L.ss_find_lines_set_device(self._h, ptr, length, _delimiter_byte(delimiter), self._how(whole_word, whole_line, invert),
                                                    _context_amount(before, "before"), _context_amount(after, "after"), st, p[0], p[1], p[2],
                                                    p[3], int(capacity), ctypes.byref(total), ctypes.byref(selected)), self._L)
        return total.value, selected.value

    def find_lines(self, haystack, before=0, after=0, delimiter=b"\n", whole_word=False, whole_line=False, invert=False, capacity=None,
                   stream=None):
        """(begin, end, number, kind) of the selected lines with ``before`` / ``after`` context lines, every line once, ascending
        (ss_find_lines_set_device); kind is 1 for a selected line and 0 for a context line."""
        import torch
        ptr, length, t = DynamicHipSearcher._device_haystack(haystack)
        dev = t.device if t is not None else torch.device("cuda", torch.cuda.current_device())
        kw = dict(before=before, after=after, delimiter=delimiter, whole_word=whole_word, whole_line=whole_line, invert=invert, stream=stream)
        hay = t if t is not None else (ptr, length)
        if capacity is None:
            capacity, _ = self.find_lines_into(hay, None, None, None, None, 0, **kw)
        out, kind = _context_arrays(capacity, dev)
        p = [out[k] if capacity else None for k in range(3)] + [kind if capacity else None]
        total, _ = self.find_lines_into(hay, p[0], p[1], p[2], p[3], capacity, **kw)
        k = min(int(capacity), total)
        return out[0, :k], out[1, :k], out[2, :k], kind[:k]

    def grep(self, haystack, before=0, after=0, delimiter=b"\n", line_numbers=False, whole_word=False, whole_line=False, invert=False,
             stream=None):
        """``grep -f FILE``'s stdout as a uint8 device tensor: ``find_lines`` followed by ``ss.format_lines`` (separators exactly when
        ``before`` or ``after`` is non-zero) - byte for byte what ``ss.grep_anyof`` gives for searchers of the same needles.  Sets
        made inside ``with ss.output_build():``."""
        L = _feature_lib(self._L, "output")
        begin, end, number, kind = self.find_lines(haystack, before, after, delimiter, whole_word, whole_line, invert, None, stream)
        return _format(L, haystack, begin, end, number, kind, delimiter, _output_flags(number, line_numbers, bool(before or after)), stream)

    # -- every occurrence, per needle (include/sliceslice_hip_setmatches.h; inside ``with ss.setmatches_build():``) --------------
    def _occurrence_how(self, whole_word):
        return (SS_BOUND_WORD if whole_word else 0) | (SS_BOUND_NOCASE if self.ignore_case else 0)

    def ranks(self):
        """The rank of every needle as given (ss_needle_set_ranks): its position in the set's sorted, deduplicated order, as an
        int64 numpy array; duplicates and needles equal after the fold share a rank."""
        L = _feature_lib(self._L, "setmatches")
        if getattr(self, "_ranks", None) is None:
            out = np.zeros(max(self._count, 1), dtype=np.uint32)
            _check(L.ss_needle_set_ranks(self._h, out.ctypes.data), L)
            self._ranks = out[:self._count].astype(np.int64)
        return self._ranks

    def _rank_maps(self, dev):
        """(ranks, the smallest given index of every rank) as int64 tensors on `dev`."""
        import torch
        maps = self.__dict__.setdefault("_maps", {})
        if dev not in maps:
            ranks = self.ranks()
            first = np.full(int(ranks.max()) + 1 if len(ranks) else 0, len(ranks), dtype=np.int64)
            np.minimum.at(first, ranks, np.arange(len(ranks), dtype=np.int64))
            maps[dev] = (torch.from_numpy(ranks).to(dev), torch.from_numpy(first).to(dev))
        return maps[dev]

    def count_async(self, haystack, d_counts, d_total, whole_word=False, stream=None):
        """ss_count_set_device_async into the caller's 8-byte device tensors: ``d_counts`` in RANK space (``info()["distinct"]``
        entries) and ``d_total`` (one entry); either may be None, not both.  Stream-ordered and capturable."""
        L = _feature_lib(self._L, "setmatches")
        ptr, length, t = DynamicHipSearcher._device_haystack(haystack)
        with _on_device_of(t):
            st = stream if stream is not None else _current_stream_handle()
            _check(L.ss_count_set_device_async(self._h, ptr, length, self._occurrence_how(whole_word), st,
                                               d_counts.data_ptr() if d_counts is not None else None,
                                               d_total.data_ptr() if d_total is not None else None), L)

    def _count_ranks(self, haystack, d_counts, whole_word, stream):
        L = _feature_lib(self._L, "setmatches")
        ptr, length, t = DynamicHipSearcher._device_haystack(haystack)
        total = _u64(0)
        with _on_device_of(t):
            st = stream if stream is not None else _current_stream_handle()
            _check(L.ss_count_set_device(self._h, ptr, length, self._occurrence_how(whole_word), st,
                                         d_counts.data_ptr() if d_counts is not None else None, ctypes.byref(total)), L)
        return total.value

    def count(self, haystack, whole_word=False, stream=None):
        """The occurrences of every needle AS GIVEN, overlapping ones included, as an int64 device tensor (ss_count_set_device: the
        counts per rank, gathered through ``ranks()``; duplicates show equal values) - what ``count`` of a searcher of each
        needle returns on the same haystack."""
        import torch
        _feature_lib(self._L, "setmatches")
        ptr, length, t = DynamicHipSearcher._device_haystack(haystack)
        dev = t.device if t is not None else torch.device("cuda", torch.cuda.current_device())
        ranks, first = self._rank_maps(dev)
        by_rank = torch.empty(max(first.numel(), 1), dtype=torch.int64, device=dev)
        self._count_ranks(t if t is not None else (ptr, length), by_rank, whole_word, stream)
        return by_rank[ranks]

    def count_total(self, haystack, whole_word=False, stream=None):
        """The number of (offset, needle) pairs: the sum of the counts of the DISTINCT needles (ss_count_set_device without bins)."""
        _feature_lib(self._L, "setmatches")
        return self._count_ranks(haystack, None, whole_word, stream)

    def find_all_into(self, haystack, d_offsets, d_ranks, capacity, whole_word=False, stream=None):
        """ss_find_all_set_device into the caller's device tensors (8-byte offsets, 4-byte RANKS; each may be None); returns the
        total number of pairs."""
        L = _feature_lib(self._L, "setmatches")
        ptr, length, t = DynamicHipSearcher._device_haystack(haystack)
        total = _u64(0)
        with _on_device_of(t):
            st = stream if stream is not None else _current_stream_handle()
            _check(L.ss_find_all_set_device(self._h, ptr, length, self._occurrence_how(whole_word), st,
                                            d_offsets.data_ptr() if d_offsets is not None else None,
                                            d_ranks.data_ptr() if d_ranks is not None else None, int(capacity), ctypes.byref(total)), L)
        return total.value

    def find_all(self, haystack, whole_word=False, capacity=None, stream=None):
        """(offsets, needle_index) of the first ``capacity`` (default: all) occurrences of the set's needles, ordered by offset and
        then by rank, as int64 device tensors; ``needle_index`` is the smallest index as given of the needle of that rank."""
        import torch
        _feature_lib(self._L, "setmatches")
        ptr, length, t = DynamicHipSearcher._device_haystack(haystack)
        dev = t.device if t is not None else torch.device("cuda", torch.cuda.current_device())
        hay = t if t is not None else (ptr, length)
        if capacity is None:
            capacity = self.find_all_into(hay, None, None, 0, whole_word, stream)
        offsets = torch.empty(max(int(capacity), 1), dtype=torch.int64, device=dev)
        rank = torch.empty(max(int(capacity), 1), dtype=torch.int32, device=dev)
        total = self.find_all_into(hay, offsets if capacity else None, rank if capacity else None, capacity, whole_word, stream)
        k = min(int(capacity), total)
        return offsets[:k], self._rank_maps(dev)[1][rank[:k].long()]

    # -- leftmost-longest selection (include/sliceslice_hip_leftmost.h; inside ``with ss.leftmost_build():``) --------------------
    def lengths(self):
        """The length of the needle of every rank (ss_needle_set_lengths) as an int64 numpy array of ``info()["distinct"]`` entries:
        what turns the ranks of ``find_all_into`` into the lengths ``ss.select_leftmost`` takes."""
        L = _feature_lib(self._L, "leftmost")
        distinct = self.info()["distinct"]
        out = np.zeros(max(distinct, 1), dtype=np.uint64)
        _check(L.ss_needle_set_lengths(self._h, out.ctypes.data), L)
        return out[:distinct].astype(np.int64)

    def count_leftmost(self, haystack, whole_word=False, stream=None):
        """int: the number of leftmost-longest, non-overlapping occurrences of the set's needles - the lines ``grep -o -F -f FILE``
        prints (ss_count_leftmost_set_device).  The word test comes before the selection."""
        L = _feature_lib(self._L, "leftmost")
        ptr, length, t = DynamicHipSearcher._device_haystack(haystack)
        c = _u64(0)
        with _on_device_of(t):
            st = stream if stream is not None else _current_stream_handle()
            _check(L.ss_count_leftmost_set_device(self._h, ptr, length, self._occurrence_how(whole_word), st, ctypes.byref(c)), L)
        return c.value

    def find_all_leftmost_into(self, haystack, d_offsets, d_ranks, capacity, whole_word=False, stream=None):
        """ss_find_all_leftmost_set_device into the caller's device tensors (8-byte offsets, 4-byte RANKS; each may be None);
        returns the number of selected occurrences."""
        L = _feature_lib(self._L, "leftmost")
        ptr, length, t = DynamicHipSearcher._device_haystack(haystack)
        total = _u64(0)
        with _on_device_of(t):
            st = stream if stream is not None else _current_stream_handle()
            _check(L.ss_find_all_leftmost_set_device(self._h, ptr, length, self._occurrence_how(whole_word), st,
                                                     d_offsets.data_ptr() if d_offsets is not None else None,
                                                     d_ranks.data_ptr() if d_ranks is not None else None, int(capacity), ctypes.byref(total)), L)
        return total.value

    def find_all_leftmost(self, haystack, whole_word=False, capacity=None, stream=None):
        """(offsets, which) of the first ``capacity`` (default: all) leftmost-longest, non-overlapping occurrences, ascending, as
        int64 device tensors; ``which`` is the smallest index as given of the selected needle, as in ``find_all``."""
        import torch
        _feature_lib(self._L, "leftmost")
        ptr, length, t = DynamicHipSearcher._device_haystack(haystack)
        dev = t.device if t is not None else torch.device("cuda", torch.cuda.current_device())
        hay = t if t is not None else (ptr, length)
        if capacity is None:
            capacity = self.find_all_leftmost_into(hay, None, None, 0, whole_word, stream)
        offsets = torch.empty(max(int(capacity), 1), dtype=torch.int64, device=dev)
        rank = torch.empty(max(int(capacity), 1), dtype=torch.int32, device=dev)
        total = self.find_all_leftmost_into(hay, offsets if capacity else None, rank if capacity else None, capacity, whole_word, stream)
        k = min(int(capacity), total)
        return offsets[:k], self._rank_maps(dev)[1][rank[:k].long()]

    def replace(self, haystack, replacements, whole_word=False, stream=None):
        """uint8 tensor on the haystack's device: the haystack with every leftmost-longest, non-overlapping occurrence replaced by
        its needle's own text - ``replacements`` is a sequence parallel to the needles as given, or a mapping needle -> text that
        holds every needle (host bytes, may be empty; needles that are equal, or equal after the set's fold, must carry equal
        texts).  ``re.sub`` over the alternation, longest first, with a function (ss_replace_set_device; one call where the output's
        length is bounded by at most twice the haystack's, else sized first)."""
        import torch
        L = _feature_lib(self._L, "leftmost")
        if hasattr(replacements, "keys"):
            given = getattr(self, "_needles", None)
            if given is None:
                raise ValueError("a mapping of replacements needs the needles of a set made by NeedleSet(needles)")
            table = {bytes(k): bytes(v) for k, v in replacements.items()}
            texts = [table[n] for n in given]
        else:
            texts = [bytes(r) for r in replacements]
        if len(texts) != self._count:
            raise ValueError("%d replacements for %d needles" % (len(texts), self._count))
        views = [_host_view(r) for r in texts]
        reps = (ctypes.c_void_p * max(self._count, 1))(*[v[1] if v[2] else None for v in views])
        lens = (ctypes.c_size_t * max(self._count, 1))(*[v[2] for v in views])
        ptr, length, t = DynamicHipSearcher._device_haystack(haystack)
        dev = t.device if t is not None else torch.device("cuda", torch.cuda.current_device())
        how = self._occurrence_how(whole_word)
        out_len, c = _u64(0), _u64(0)
        # One pass where the output's length is bounded cheaply: no selection can add more than the longest text less the shortest
        # needle, so texts that add nothing bound it by the haystack's length, and others by the pairs' count (one scan) times
        # that growth.  The buffer is taken from the bound when it is at most twice the haystack; else the call sizes it first.
        given = getattr(self, "_needles", None)
        grow = max(0, max(len(r) for r in texts) - min(len(n) for n in given)) if given and all(given) else None
        with _on_device_of(t):
            st = stream if stream is not None else _current_stream_handle()
            bound = None if grow is None else length if grow == 0 or length == 0 else \
                length + grow * self.count_total(t if t is not None else (ptr, length), whole_word, st)
            if bound is not None and bound <= 2 * length + (1 << 20):
                out = torch.empty(max(bound, 1), dtype=torch.uint8, device=dev)
                _check(L.ss_replace_set_device(self._h, ptr, length, how, reps, lens, self._count, st, out.data_ptr(), bound,
                                               ctypes.byref(out_len), ctypes.byref(c)), L)
                if out_len.value <= bound:                      # (always: the bound holds)
                    return out[:out_len.value]
            _check(L.ss_replace_set_device(self._h, ptr, length, how, reps, lens, self._count, st, None, 0, ctypes.byref(out_len),
                                           ctypes.byref(c)), L)
            out = torch.empty(max(out_len.value, 1), dtype=torch.uint8, device=dev)
            if out_len.value:
                _check(L.ss_replace_set_device(self._h, ptr, length, how, reps, lens, self._count, st, out.data_ptr(), out_len.value,
                                               ctypes.byref(out_len), ctypes.byref(c)), L)
        return out[:min(out_len.value, out.numel() if out_len.value else 0)]

    def close(self):
        h, self._h = getattr(self, "_h", None), None
        L = getattr(self, "_L", None)
        if h and L is not None and _lib is not None:
            L.ss_needle_set_free(h)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def parse_hex(text):
    """(value, mask) bytes of a hex pattern such as ``"48 8b ?? 4?"`` (ss_masked_parse_hex: tokens of two characters separated by
    optional blanks, each character a hex digit of either case or ``?``).  Host only; inside ``with ss.masked_build():``."""
    L = _feature_lib(lib(), "masked")
    raw = text.encode("latin-1") if isinstance(text, str) else bytes(text)
    if b"\0" in raw:
        raise SlicesliceError(SS_ERR_ARGUMENT, "ss_masked_parse_hex: column %d: a NUL is neither a hex digit nor '?'" % (raw.index(b"\0") + 1))
    n = _sz(0)
    _check(L.ss_masked_parse_hex(raw, None, None, 0, ctypes.byref(n)), L)
    value, mask = np.zeros(max(n.value, 1), dtype=np.uint8), np.zeros(max(n.value, 1), dtype=np.uint8)
    _check(L.ss_masked_parse_hex(raw, value.ctypes.data, mask.ctypes.data, n.value, ctypes.byref(n)), L)
    return value[:n.value].tobytes(), mask[:n.value].tobytes()


def masked_choose_filter(value, mask=None, hist=None):
    """(anchor, distance) of ss_masked_choose_filter: the two pattern positions the masked kernel tests in registers (distance 0:
    one).  ``hist``: 256 counts of the haystack's bytes, or None for the static costs.  Host only; inside ``with ss.masked_build():``."""
    L = _feature_lib(lib(), "masked")
    v = np.frombuffer(bytes(value), dtype=np.uint8)
    m = np.frombuffer(bytes(mask), dtype=np.uint8) if mask is not None else None
    if m is not None and m.size != v.size:
        raise ValueError("value holds %d bytes and mask %d" % (v.size, m.size))
    h = np.ascontiguousarray(hist, dtype=np.uint64) if hist is not None else None
    if h is not None and h.size != 256:
        raise ValueError("a histogram holds 256 counts, got %d" % h.size)
    a, d = _sz(0), _sz(0)
    _check(L.ss_masked_choose_filter(v.ctypes.data if v.size else None, m.ctypes.data if m is not None and m.size else None, v.size,
                                     h.ctypes.data if h is not None else None, ctypes.byref(a), ctypes.byref(d)), L)
    return a.value, d.value


class MaskedPattern:
    """A fixed-length byte pattern with a mask per byte (ss_masked_new, inside ``with ss.masked_build():``) on the current device:
    position p matches when ``(hay[p + i] & mask[i]) == value[i]`` for every i (include/sliceslice_hip_masked.h has the rule).
    ``mask=None`` means all 0xFF.  The methods follow ``NeedleSet``'s forms."""

    def __init__(self, value, mask=None):
        self._h = None
        self._L = L = _feature_lib(lib(), "masked")
        v = np.frombuffer(bytes(value), dtype=np.uint8)
        m = np.frombuffer(bytes(mask), dtype=np.uint8) if mask is not None else None
        if m is not None and m.size != v.size:
            raise ValueError("value holds %d bytes and mask %d" % (v.size, m.size))
        h = ctypes.c_void_p()
        _check(L.ss_masked_new(v.ctypes.data if v.size else None, m.ctypes.data if m is not None and m.size else None, v.size, ctypes.byref(h)), L)
        self._h = h
        self.mask = m.tobytes() if m is not None else b"\xff" * v.size
        self.value = bytes(a & b for a, b in zip(v.tobytes(), self.mask))

    @classmethod
    def from_hex(cls, text):
        """The pattern of a YARA / ClamAV style hex string: ``MaskedPattern.from_hex("48 8b ?? 4?")``."""
        return cls(*parse_hex(text))

    @classmethod
    def from_bytes(cls, data, ignore_case=False):
        """The pattern of a literal; ``ignore_case``: the letters A-Z / a-z get mask 0xDF, which is exact for them and touches
        no other byte."""
        data = bytes(data)
        mask = bytes(0xDF if ignore_case and (0x41 <= b <= 0x5A or 0x61 <= b <= 0x7A) else 0xFF for b in data)
        return cls(data, mask)

    def info(self, delimiter=None):
        """dict of ss_masked_info: n, anchor, distance, full, partial, wild, accepts_delimiter (for ``delimiter``, if one is given)."""
        words = (ctypes.c_uint64 * len(MASKED_STATS))()
        _check(self._L.ss_masked_info(self._h, -1 if delimiter is None else _delimiter_byte(delimiter), words), self._L)
        d = dict(zip(MASKED_STATS, (int(w) for w in words)))
        del d["reserved"]
        return d

    def count(self, haystack, stream=None):
        """int: the occurrences, overlapping ones included (ss_count_masked_device)."""
        ptr, length, t = DynamicHipSearcher._device_haystack(haystack)
        c = _u64(0)
        with _on_device_of(t):
            st = stream if stream is not None else _current_stream_handle()
            _check(self._L.ss_count_masked_device(self._h, ptr, length, st, ctypes.byref(c)), self._L)
        return c.value

    def count_async(self, haystack, out=None, stream=None):
        """ss_count_masked_device_async into ``out`` (a one-element int64 device tensor, made when None) and returns it:
        stream-ordered, no wait, capturable into a graph."""
        import torch
        ptr, length, t = DynamicHipSearcher._device_haystack(haystack)
        if out is None:
            out = torch.empty(1, dtype=torch.int64, device=t.device if t is not None else torch.device("cuda", torch.cuda.current_device()))
        with _on_device_of(t):
            st = stream if stream is not None else _current_stream_handle()
            _check(self._L.ss_count_masked_device_async(self._h, ptr, length, st, out.data_ptr()), self._L)
        return out

    def find_all_into(self, haystack, out, capacity=None, stream=None):
        """ss_find_all_masked_device into the caller's 8-byte device tensor (None with capacity 0); returns the total."""
        ptr, length, t = DynamicHipSearcher._device_haystack(haystack)
        if capacity is None:
            capacity = out.numel() if out is not None else 0
        total = _u64(0)
        with _on_device_of(t):
            st = stream if stream is not None else _current_stream_handle()
            _check(self._L.ss_find_all_masked_device(self._h, ptr, length, st, out.data_ptr() if out is not None else None, int(capacity),
                                                     ctypes.byref(total)), self._L)
        return total.value

    def find_all(self, haystack, capacity=None, stream=None):
        """int64 device tensor: the first ``capacity`` (default: all, counted first) occurrence offsets, ascending."""
        import torch
        ptr, length, t = DynamicHipSearcher._device_haystack(haystack)
        dev = t.device if t is not None else torch.device("cuda", torch.cuda.current_device())
        hay = t if t is not None else (ptr, length)
        if capacity is None:
            capacity = self.find_all_into(hay, None, 0, stream)
        out = torch.empty(max(int(capacity), 1), dtype=torch.int64, device=dev)
        total = self.find_all_into(hay, out if capacity else None, int(capacity), stream)
        return out[:min(int(capacity), total)]

    def count_lines(self, haystack, delimiter=b"\n", stream=None):
        """int: the lines that hold an occurrence wholly inside them (ss_count_lines_masked_device)."""
        ptr, length, t = DynamicHipSearcher._device_haystack(haystack)
        c = _u64(0)
        with _on_device_of(t):
            st = stream if stream is not None else _current_stream_handle()
            _check(self._L.ss_count_lines_masked_device(self._h, ptr, length, _delimiter_byte(delimiter), st, ctypes.byref(c)), self._L)
        return c.value

    def find_lines_into(self, haystack, d_begin, d_end, d_number, capacity, delimiter=b"\n", stream=None):
        """ss_find_lines_masked_device into the caller's 8-byte device tensors (each may be None); returns the total."""
        ptr, length, t = DynamicHipSearcher._device_haystack(haystack)
        total = _u64(0)
        with _on_device_of(t):
            st = stream if stream is not None else _current_stream_handle()
            p = [x.data_ptr() if x is not None else None for x in (d_begin, d_end, d_number)]
            _check(self._L.ss_find_lines_masked_device(self._h, ptr, length, _delimiter_byte(delimiter), st, p[0], p[1], p[2], int(capacity),
                                                       ctypes.byref(total)), self._L)
        return total.value

    def find_lines(self, haystack, delimiter=b"\n", capacity=None, stream=None):
        """(begin, end, number) int64 device tensors of the first ``capacity`` (default: all, counted first) matching lines,
        ascending - the records of ``DynamicHipSearcher.find_lines``."""
        import torch
        ptr, length, t = DynamicHipSearcher._device_haystack(haystack)
        dev = t.device if t is not None else torch.device("cuda", torch.cuda.current_device())
        hay = t if t is not None else (ptr, length)
        if capacity is None:
            capacity = self.count_lines(hay, delimiter, stream)
        out = torch.empty((3, max(int(capacity), 1)), dtype=torch.int64, device=dev)
        p = [out[k] if capacity else None for k in range(3)]
        total = self.find_lines_into(hay, p[0], p[1], p[2], int(capacity), delimiter, stream)
        k = min(int(capacity), total)
        return out[0, :k], out[1, :k], out[2, :k]

    def close(self):
        h, self._h = getattr(self, "_h", None), None
        L = getattr(self, "_L", None)
        if h and L is not None and _lib is not None:
            L.ss_masked_free(h)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _class_sets(sets):
    """``sets`` as a contiguous (n, 4) uint64 array: 256 bits per position, byte b is bit b & 63 of word b >> 6."""
    a = np.ascontiguousarray(sets, dtype=np.uint64)
    if a.ndim != 2 or a.shape[1] != 4:
        raise ValueError("sets are an (n, 4) array of 64-bit words, got shape %r" % (a.shape,))
    return a


def parse_classes(text, ignore_case=False):
    """(n, 4) uint64 array: the set of every position of a pattern such as ``r"[0-9A-F]{4}H"`` (ss_classes_parse: the strict subset
    of Python ``re`` byte patterns under re.DOTALL that include/sliceslice_hip_classes.h lays down).  Host only; inside
    ``with ss.classes_build():``."""
    L = _feature_lib(lib(), "classes")
    raw = text.encode("latin-1") if isinstance(text, str) else bytes(text)
    if b"\0" in raw:
        raise SlicesliceError(SS_ERR_ARGUMENT, "ss_classes_parse: column %d: a NUL ends the text: write \\x00" % (raw.index(b"\0") + 1))
    n = _sz(0)
    _check(L.ss_classes_parse(raw, int(bool(ignore_case)), None, 0, ctypes.byref(n)), L)
    sets = np.zeros((max(n.value, 1), 4), dtype=np.uint64)
    _check(L.ss_classes_parse(raw, int(bool(ignore_case)), sets.ctypes.data, n.value, ctypes.byref(n)), L)
    return sets[:n.value]


def classes_cover(sets):
    """(value, mask) bytes: the tightest cover of every position's set (ss_classes_cover).  Host only; inside
    ``with ss.classes_build():``."""
    L = _feature_lib(lib(), "classes")
    a = _class_sets(sets)
    value, mask = np.zeros(max(len(a), 1), dtype=np.uint8), np.zeros(max(len(a), 1), dtype=np.uint8)
    _check(L.ss_classes_cover(a.ctypes.data if len(a) else None, len(a), value.ctypes.data, mask.ctypes.data), L)
    return value[:len(a)].tobytes(), mask[:len(a)].tobytes()


class ClassPattern:
    """A fixed-length pattern whose positions are sets of bytes (ss_classes_new, inside ``with ss.classes_build():``) on the current
    device: position p matches when ``hay[p + i]`` is in set i for every i (include/sliceslice_hip_classes.h has the rule and the
    pattern language of ``text``).  The methods are ``MaskedPattern``'s."""

    def __init__(self, text, ignore_case=False):
        self._h = None
        self._L = _feature_lib(lib(), "classes")
        self._make(parse_classes(text, ignore_case))

    def _make(self, sets):
        L = self._L
        h = ctypes.c_void_p()
        _check(L.ss_classes_new(sets.ctypes.data if len(sets) else None, len(sets), ctypes.byref(h)), L)
        self._h = h
        self.sets = sets

    @classmethod
    def from_sets(cls, sets):
        """The pattern of an (n, 4) array of 64-bit words: 256 bits per position."""
        self = cls.__new__(cls)
        self._h = None
        self._L = _feature_lib(lib(), "classes")
        self._make(_class_sets(sets).copy())
        return self

    @classmethod
    def from_masked(cls, value, mask=None):
        """The pattern that accepts at position i the bytes b with ``(b & mask[i]) == (value[i] & mask[i])``: what
        ``MaskedPattern(value, mask)`` accepts.  No position of it is inexact."""
        v = np.frombuffer(bytes(value), dtype=np.uint8)
        m = np.frombuffer(bytes(mask), dtype=np.uint8) if mask is not None else np.full(v.size, 0xFF, dtype=np.uint8)
        if m.size != v.size:
            raise ValueError("value holds %d bytes and mask %d" % (v.size, m.size))
        b = np.arange(256, dtype=np.uint8)
        member = (b[None, :] & m[:, None]) == (v & m)[:, None]
        bits = np.packbits(member, axis=1, bitorder="little")
        return cls.from_sets(np.ascontiguousarray(bits).view("<u8").astype(np.uint64).reshape(v.size, 4))

    @classmethod
    def from_bytes(cls, data, ignore_case=False):
        """The pattern of a literal; ``ignore_case``: the letters A-Z / a-z accept either case."""
        data = bytes(data)
        return cls.from_masked(data, bytes(0xDF if ignore_case and (0x41 <= b <= 0x5A or 0x61 <= b <= 0x7A) else 0xFF for b in data))

    def __len__(self):
        return len(self.sets)

    def info(self, delimiter=None):
        """dict of ss_classes_info: n, anchor, distance, single, masked, inexact, distinct, accepts_delimiter (for ``delimiter``, if
        one is given)."""
        words = (ctypes.c_uint64 * len(CLASSES_STATS))()
        _check(self._L.ss_classes_info(self._h, -1 if delimiter is None else _delimiter_byte(delimiter), words), self._L)
        return dict(zip(CLASSES_STATS, (int(w) for w in words)))

    def count(self, haystack, stream=None):
        """int: the occurrences, overlapping ones included (ss_count_classes_device)."""
        ptr, length, t = DynamicHipSearcher._device_haystack(haystack)
        c = _u64(0)
        with _on_device_of(t):
            st = stream if stream is not None else _current_stream_handle()
            _check(self._L.ss_count_classes_device(self._h, ptr, length, st, ctypes.byref(c)), self._L)
        return c.value

    def count_async(self, haystack, out=None, stream=None):
        """ss_count_classes_device_async into ``out`` (a one-element int64 device tensor, made when None) and returns it:
        stream-ordered, no wait, capturable into a graph."""
        import torch
        ptr, length, t = DynamicHipSearcher._device_haystack(haystack)
        if out is None:
            out = torch.empty(1, dtype=torch.int64, device=t.device if t is not None else torch.device("cuda", torch.cuda.current_device()))
        with _on_device_of(t):
            st = stream if stream is not None else _current_stream_handle()
            _check(self._L.ss_count_classes_device_async(self._h, ptr, length, st, out.data_ptr()), self._L)
        return out

    def find_all_into(self, haystack, out, capacity=None, stream=None):
        """ss_find_all_classes_device into the caller's 8-byte device tensor (None with capacity 0); returns the total."""
        ptr, length, t = DynamicHipSearcher._device_haystack(haystack)
        if capacity is None:
            capacity = out.numel() if out is not None else 0
        total = _u64(0)
        with _on_device_of(t):
            st = stream if stream is not None else _current_stream_handle()
            _check(self._L.ss_find_all_classes_device(self._h, ptr, length, st, out.data_ptr() if out is not None else None, int(capacity),
                                                      ctypes.byref(total)), self._L)
        return total.value

    def find_all(self, haystack, capacity=None, stream=None):
        """int64 device tensor: the first ``capacity`` (default: all, counted first) occurrence offsets, ascending."""
        import torch
        ptr, length, t = DynamicHipSearcher._device_haystack(haystack)
        dev = t.device if t is not None else torch.device("cuda", torch.cuda.current_device())
        hay = t if t is not None else (ptr, length)
        if capacity is None:
            capacity = self.find_all_into(hay, None, 0, stream)
        out = torch.empty(max(int(capacity), 1), dtype=torch.int64, device=dev)
        total = self.find_all_into(hay, out if capacity else None, int(capacity), stream)
        return out[:min(int(capacity), total)]

    def count_lines(self, haystack, delimiter=b"\n", stream=None):
        """int: the lines that hold an occurrence wholly inside them (ss_count_lines_classes_device)."""
        ptr, length, t = DynamicHipSearcher._device_haystack(haystack)
        c = _u64(0)
        with _on_device_of(t):
            st = stream if stream is not None else _current_stream_handle()
            _check(self._L.ss_count_lines_classes_device(self._h, ptr, length, _delimiter_byte(delimiter), st, ctypes.byref(c)), self._L)
        return c.value

    def find_lines_into(self, haystack, d_begin, d_end, d_number, capacity, delimiter=b"\n", stream=None):
        """ss_find_lines_classes_device into the caller's 8-byte device tensors (each may be None); returns the total."""
        ptr, length, t = DynamicHipSearcher._device_haystack(haystack)
        total = _u64(0)
        with _on_device_of(t):
            st = stream if stream is not None else _current_stream_handle()
            p = [x.data_ptr() if x is not None else None for x in (d_begin, d_end, d_number)]
            _check(self._L.ss_find_lines_classes_device(self._h, ptr, length, _delimiter_byte(delimiter), st, p[0], p[1], p[2], int(capacity),
                                                        ctypes.byref(total)), self._L)
        return total.value

    def find_lines(self, haystack, delimiter=b"\n", capacity=None, stream=None):
        """(begin, end, number) int64 device tensors of the first ``capacity`` (default: all, counted first) matching lines,
        ascending - the records of ``DynamicHipSearcher.find_lines``."""
        import torch
        ptr, length, t = DynamicHipSearcher._device_haystack(haystack)
        dev = t.device if t is not None else torch.device("cuda", torch.cuda.current_device())
        hay = t if t is not None else (ptr, length)
        if capacity is None:
            capacity = self.count_lines(hay, delimiter, stream)
        out = torch.empty((3, max(int(capacity), 1)), dtype=torch.int64, device=dev)
        p = [out[k] if capacity else None for k in range(3)]
        total = self.find_lines_into(hay, p[0], p[1], p[2], int(capacity), delimiter, stream)
        k = min(int(capacity), total)
        return out[0, :k], out[1, :k], out[2, :k]

    def close(self):
        h, self._h = getattr(self, "_h", None), None
        L = getattr(self, "_L", None)
        if h and L is not None and _lib is not None:
            L.ss_classes_free(h)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def parse_runs(text, ignore_case=False):
    """(set, min_len, max_len): the four 64-bit words of the class and the bounds (``max_len`` None: no maximum) of a run pattern
    such as ``r"\\w+"`` or ``r"[0-9]{3,}"`` (ss_runs_parse: ONE item of the classes language and one of ``+ {k} {k,} {k,m}``,
    include/sliceslice_hip_runs.h).  Host only; inside ``with ss.runs_build():``."""
    L = _feature_lib(lib(), "runs")
    raw = text.encode("latin-1") if isinstance(text, str) else bytes(text)
    if b"\0" in raw:
        raise SlicesliceError(SS_ERR_ARGUMENT, "ss_runs_parse: column %d: a NUL ends the text: write \\x00" % (raw.index(b"\0") + 1))
    words = np.zeros(4, dtype=np.uint64)
    lo, hi = _u64(0), _u64(0)
    _check(L.ss_runs_parse(raw, int(bool(ignore_case)), words.ctypes.data, ctypes.byref(lo), ctypes.byref(hi)), L)
    return words, int(lo.value), int(hi.value) or None


class RunPattern:
    """The maximal runs of one byte class whose length lies in ``[min_len, max_len]`` (ss_runs_new, inside ``with ss.runs_build():``)
    on the current device: ``\\w+``, ``[0-9]{3,}``, ``[A-Z]{2,5}`` (include/sliceslice_hip_runs.h has the rule and the language of
    ``text``).  A run that is too long is not selected and no run is chopped."""

    def __init__(self, text, ignore_case=False):
        self._h = None
        self._L = _feature_lib(lib(), "runs")
        words, lo, hi = parse_runs(text, ignore_case)
        self._make(words, lo, hi, False)

    def _make(self, words, min_len, max_len, bitmap):
        L = self._L
        h = ctypes.c_void_p()
        _check(L.ss_runs_new(words.ctypes.data, int(min_len), int(max_len or 0), SS_RUNS_BITMAP if bitmap else 0, ctypes.byref(h)), L)
        self._h = h
        self.set, self.min_len, self.max_len = words, int(min_len), (int(max_len) if max_len else None)

    @classmethod
    def from_set(cls, set_words, min_len=1, max_len=None, bitmap=False):
        """The pattern of four 64-bit words (byte b is bit ``b & 63`` of word ``b >> 6``); ``bitmap``: force the bitmap path."""
        self = cls.__new__(cls)
        self._h = None
        self._L = _feature_lib(lib(), "runs")
        words = np.ascontiguousarray(np.asarray(set_words, dtype=np.uint64).reshape(-1))
        if words.shape != (4,):
            raise ValueError("a set is four 64-bit words, got shape %r" % (np.asarray(set_words).shape,))
        self._make(words.copy(), min_len, max_len, bitmap)
        return self

    def info(self, delimiter=None):
        """dict of ss_runs_info: min_len, max_len (0: none), members, ranges, path (0: range tests, 1: the bitmap),
        accepts_delimiter (for ``delimiter``, if one is given)."""
        words = (ctypes.c_uint64 * len(RUNS_STATS))()
        _check(self._L.ss_runs_info(self._h, -1 if delimiter is None else _delimiter_byte(delimiter), words), self._L)
        return dict(zip(RUNS_STATS, (int(w) for w in words)))

    def count(self, haystack, stream=None):
        """int: the selected runs (ss_count_runs_device)."""
        ptr, length, t = DynamicHipSearcher._device_haystack(haystack)
        c = _u64(0)
        with _on_device_of(t):
            st = stream if stream is not None else _current_stream_handle()
            _check(self._L.ss_count_runs_device(self._h, ptr, length, st, ctypes.byref(c)), self._L)
        return c.value

    def count_async(self, haystack, out=None, stream=None):
        """ss_count_runs_device_async into ``out`` (a one-element int64 device tensor, made when None) and returns it:
        stream-ordered, no wait, capturable into a graph."""
        import torch
        ptr, length, t = DynamicHipSearcher._device_haystack(haystack)
        if out is None:
            out = torch.empty(1, dtype=torch.int64, device=t.device if t is not None else torch.device("cuda", torch.cuda.current_device()))
        with _on_device_of(t):
            st = stream if stream is not None else _current_stream_handle()
            _check(self._L.ss_count_runs_device_async(self._h, ptr, length, st, out.data_ptr()), self._L)
        return out

    def find_all_into(self, haystack, d_begin, d_end, capacity=None, stream=None):
        """ss_find_all_runs_device into the caller's 8-byte device tensors (either may be None; both with capacity 0); returns the
        total."""
        ptr, length, t = DynamicHipSearcher._device_haystack(haystack)
        if capacity is None:
            capacity = min(x.numel() for x in (d_begin, d_end) if x is not None) if (d_begin is not None or d_end is not None) else 0
        total = _u64(0)
        with _on_device_of(t):
            st = stream if stream is not None else _current_stream_handle()
            p = [x.data_ptr() if x is not None else None for x in (d_begin, d_end)]
            _check(self._L.ss_find_all_runs_device(self._h, ptr, length, st, p[0], p[1], int(capacity), ctypes.byref(total)), self._L)
        return total.value

    def find_all(self, haystack, capacity=None, stream=None):
        """(begin, end) int64 device tensors: the first ``capacity`` (default: all, counted first) selected runs, ascending."""
        import torch
        ptr, length, t = DynamicHipSearcher._device_haystack(haystack)
        dev = t.device if t is not None else torch.device("cuda", torch.cuda.current_device())
        hay = t if t is not None else (ptr, length)
        if capacity is None:
            capacity = self.find_all_into(hay, None, None, 0, stream)
        out = torch.empty((2, max(int(capacity), 1)), dtype=torch.int64, device=dev)
        total = self.find_all_into(hay, out[0] if capacity else None, out[1] if capacity else None, int(capacity), stream)
        k = min(int(capacity), total)
        return out[0, :k], out[1, :k]

    def count_lines(self, haystack, delimiter=b"\n", stream=None):
        """int: the lines that hold a selected run; the delimiter is never a member (ss_count_lines_runs_device)."""
        ptr, length, t = DynamicHipSearcher._device_haystack(haystack)
        c = _u64(0)
        with _on_device_of(t):
            st = stream if stream is not None else _current_stream_handle()
            _check(self._L.ss_count_lines_runs_device(self._h, ptr, length, _delimiter_byte(delimiter), st, ctypes.byref(c)), self._L)
        return c.value

    def find_lines_into(self, haystack, d_begin, d_end, d_number, capacity, delimiter=b"\n", stream=None):
        """ss_find_lines_runs_device into the caller's 8-byte device tensors (each may be None); returns the total."""
        ptr, length, t = DynamicHipSearcher._device_haystack(haystack)
        total = _u64(0)
        with _on_device_of(t):
            st = stream if stream is not None else _current_stream_handle()
            p = [x.data_ptr() if x is not None else None for x in (d_begin, d_end, d_number)]
            _check(self._L.ss_find_lines_runs_device(self._h, ptr, length, _delimiter_byte(delimiter), st, p[0], p[1], p[2], int(capacity),
                                                     ctypes.byref(total)), self._L)
        return total.value

    def find_lines(self, haystack, delimiter=b"\n", capacity=None, stream=None):
        """(begin, end, number) int64 device tensors of the first ``capacity`` (default: all, counted first) matching lines,
        ascending - the records of ``DynamicHipSearcher.find_lines``."""
        import torch
        ptr, length, t = DynamicHipSearcher._device_haystack(haystack)
        dev = t.device if t is not None else torch.device("cuda", torch.cuda.current_device())
        hay = t if t is not None else (ptr, length)
        if capacity is None:
            capacity = self.count_lines(hay, delimiter, stream)
        out = torch.empty((3, max(int(capacity), 1)), dtype=torch.int64, device=dev)
        p = [out[k] if capacity else None for k in range(3)]
        total = self.find_lines_into(hay, p[0], p[1], p[2], int(capacity), delimiter, stream)
        k = min(int(capacity), total)
        return out[0, :k], out[1, :k], out[2, :k]

    # -- the selected runs replaced or deleted (libsliceslice_hip_rewrite.so: patterns made inside `with ss.rewrite_build():`) ------
    def replace_into(self, haystack, text, d_out, delimiter=None, stream=None):
        """ss_replace_runs_device into the caller's uint8 device tensor ``d_out`` (None: the sizing call, one pass); returns
        ``(out_len, count)``.  Nothing is written where ``d_out`` holds fewer than ``out_len`` bytes.  ``text`` is host bytes, at
        most SS_REWRITE_MAX_TEXT of them, and may be empty; ``delimiter`` (None: none) is a byte that is never a member here."""
        L = _feature_lib(self._L, "rewrite")
        ptr, length, t = DynamicHipSearcher._device_haystack(haystack)
        keep, addr, rn = _host_view(bytes(text))
        out_len, c = _u64(0), _u64(0)
        with _on_device_of(t):
            st = stream if stream is not None else _current_stream_handle()
            _check(L.ss_replace_runs_device(self._h, ptr, length, -1 if delimiter is None else _delimiter_byte(delimiter), addr, rn, st,
                                            d_out.data_ptr() if d_out is not None else None, d_out.numel() if d_out is not None else 0,
                                            ctypes.byref(out_len), ctypes.byref(c)), L)
        return out_len.value, c.value

    def replace(self, haystack, text, delimiter=None, stream=None):
        """uint8 tensor on the haystack's device: the haystack with every selected run replaced by ``text`` - ``re.sub`` of the
        pattern.  A text of at most ``min_len`` bytes cannot make the output longer than the view: one call into a buffer of the
        view's size; any other text is sized first."""
        import torch
        _feature_lib(self._L, "rewrite")
        ptr, length, t = DynamicHipSearcher._device_haystack(haystack)
        dev = t.device if t is not None else torch.device("cuda", torch.cuda.current_device())
        hay = t if t is not None else (ptr, length)
        text = bytes(text)
        if len(text) <= self.min_len:
            out = torch.empty(max(length, 1), dtype=torch.uint8, device=dev)
            out_len, _ = self.replace_into(hay, text, out[:length], delimiter, stream)
            return out[:out_len]
        out_len, _ = self.replace_into(hay, text, None, delimiter, stream)
        out = torch.empty(max(out_len, 1), dtype=torch.uint8, device=dev)
        if out_len:
            out_len, _ = self.replace_into(hay, text, out[:out_len], delimiter, stream)
        return out[:min(out_len, out.numel() if out_len else 0)]

    def delete(self, haystack, delimiter=None, stream=None):
        """``replace`` with the empty text: the haystack without its selected runs (``tr -d``)."""
        return self.replace(haystack, b"", delimiter, stream)

    # -- the selected runs grouped and counted (libsliceslice_hip_groups.so: patterns made inside `with ss.groups_build():`) --------
    def groups_into(self, haystack, d_begin, d_end, d_count, capacity=None, ignore_case=False, stream=None, weak_hash=False):
        """ss_group_runs_device into the caller's 8-byte device tensors (each may be None; capacity: default the shortest of them,
        0 where all are None); returns ``(groups, tokens)``."""
        L = _feature_lib(self._L, "groups")
        ptr, length, t = DynamicHipSearcher._device_haystack(haystack)
        given = [x for x in (d_begin, d_end, d_count) if x is not None]
        if capacity is None:
            capacity = min(x.numel() for x in given) if given else 0
        groups, tokens = _u64(0), _u64(0)
        with _on_device_of(t):
            st = stream if stream is not None else _current_stream_handle()
            p = [x.data_ptr() if x is not None and x.numel() else None for x in (d_begin, d_end, d_count)]
            _check(L.ss_group_runs_device(self._h, ptr, length, _groups_flags(ignore_case, weak_hash), st, p[0], p[1], p[2], int(capacity),
                                          ctypes.byref(groups), ctypes.byref(tokens)), L)
        return groups.value, tokens.value

    def groups(self, haystack, ignore_case=False, stream=None, weak_hash=False):
        """(begin, end, count) int64 device tensors, one row per DISTINCT selected run in first-occurrence order: the first run
        with those bytes and how many there are - ``collections.Counter(re.findall(...))`` without leaving the device
        (ss_group_runs_device with room for _GROUPS_ROWS rows: one call for a vocabulary of that size; a larger one REPEATS THE
        WHOLE CALL, sized - call ``groups_into`` with room for every row where that matters).  ``ss.gather_ranges(haystack, begin, end, b"\\n")`` prints the vocabulary.  ``ignore_case`` folds ASCII letters
        before keys are compared."""
        import torch
        _feature_lib(self._L, "groups")
        ptr, length, t = DynamicHipSearcher._device_haystack(haystack)
        dev = t.device if t is not None else torch.device("cuda", torch.cuda.current_device())
        hay = t if t is not None else (ptr, length)
        out = torch.empty((3, _GROUPS_ROWS), dtype=torch.int64, device=dev)
        total, _ = self.groups_into(hay, out[0], out[1], out[2], _GROUPS_ROWS, ignore_case, stream, weak_hash)
        if total > _GROUPS_ROWS:
            out = torch.empty((3, total), dtype=torch.int64, device=dev)
            again, _ = self.groups_into(hay, out[0], out[1], out[2], total, ignore_case, stream, weak_hash)
            total = min(total, again)
        return out[0, :total], out[1, :total], out[2, :total]

    def most_common(self, haystack, k=None, ignore_case=False, stream=None):
        """(begin, end, count) of the ``k`` (None: all) most frequent distinct runs, most frequent first, ties in first-occurrence
        order - ``Counter.most_common(k)``: ``groups`` and a stable descending sort of the counts on the device."""
        import torch
        begin, end, count = self.groups(haystack, ignore_case, stream)
        order = torch.sort(count, descending=True, stable=True).indices
        if k is not None:
            order = order[:max(int(k), 0)]
        return begin[order], end[order], count[order]

    def close(self):
        h, self._h = getattr(self, "_h", None), None
        L = getattr(self, "_L", None)
        if h and L is not None and _lib is not None:
            L.ss_runs_free(h)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def parse_fields(text):
    """(first, last): cut's single range ``K``, ``K-``, ``K-M`` or ``-M`` (ss_fields_parse, include/sliceslice_hip_fields.h);
    ``last`` 0 means "to the line's end".  A comma list is refused: make one call per range.  Host only; inside
    ``with ss.fields_build():``."""
    L = _feature_lib(lib(), "fields")
    raw = text.encode("latin-1") if isinstance(text, str) else bytes(text)
    if b"\0" in raw:
        raise SlicesliceError(SS_ERR_ARGUMENT, "ss_fields_parse: column %d: a NUL ends the text" % (raw.index(b"\0") + 1))
    lo, hi = _u64(0), _u64(0)
    _check(L.ss_fields_parse(raw, ctypes.byref(lo), ctypes.byref(hi)), L)
    return int(lo.value), int(hi.value)


class FieldSelector:
    """Fields ``first .. last`` of every line (ss_fields_new, inside ``with ss.fields_build():``) on the current device:
    ``cut -d, -f3`` is ``FieldSelector(b",", 3)``, ``awk '{print $2}'`` is ``FieldSelector(r"[ \\t]", 2, merge=True)``
    (include/sliceslice_hip_fields.h has the rule).  ``separator``: a bytes object of members, ONE item of the classes language as a
    str (``r"[ \\t]"``, ``","``), or four 64-bit words.  ``last=None`` means ``last = first``, ``last=0`` "to the line's end".
    ``keep_short``: an empty record for every line that is not selected, so that record k is line k + 1."""

    def __init__(self, separator, first, last=None, merge=False, keep_short=False):
        self._h = None
        L = self._L = _feature_lib(lib(), "fields")
        if isinstance(separator, (bytes, bytearray)):
            words = np.zeros(4, dtype=np.uint64)
            for b in bytes(separator):
                words[b >> 6] |= np.uint64(1 << (b & 63))
        elif isinstance(separator, str):
            sets = parse_classes(separator)
            if len(sets) != 1:
                raise ValueError("the separator is ONE item of the classes language, %r has %d" % (separator, len(sets)))
            words = sets[0].copy()
        else:
            words = np.ascontiguousarray(np.asarray(separator, dtype=np.uint64).reshape(-1)).copy()
            if words.shape != (4,):
                raise ValueError("a set is four 64-bit words, got shape %r" % (np.asarray(separator).shape,))
        first = int(first)
        last = first if last is None else int(last)
        mode = SS_FIELDS_MERGE if merge else SS_FIELDS_EACH
        flags = SS_FIELDS_KEEP_SHORT if keep_short else 0
        h = ctypes.c_void_p()
        _check(L.ss_fields_new(words.ctypes.data, mode, first, last, flags, ctypes.byref(h)), L)
        self._h = h
        self.set, self.first, self.last, self.merge, self.keep_short = words, first, last, bool(merge), bool(keep_short)

    def info(self, delimiter=None):
        """dict of ss_fields_info: mode, first, last (0: to the line's end), flags, members, accepts_delimiter (for ``delimiter``,
        if one is given)."""
        words = (ctypes.c_uint64 * len(FIELDS_STATS))()
        _check(self._L.ss_fields_info(self._h, -1 if delimiter is None else _delimiter_byte(delimiter), words), self._L)
        return dict(zip(FIELDS_STATS, (int(w) for w in words)))

    def count(self, haystack, delimiter=b"\n", stream=None):
        """(selected, total): the lines that have field ``first``, and all lines (ss_count_fields_device); one pass."""
        ptr, length, t = DynamicHipSearcher._device_haystack(haystack)
        sel, tot = _u64(0), _u64(0)
        with _on_device_of(t):
            st = stream if stream is not None else _current_stream_handle()
            _check(self._L.ss_count_fields_device(self._h, ptr, length, _delimiter_byte(delimiter), st, ctypes.byref(sel), ctypes.byref(tot)), self._L)
        return sel.value, tot.value

    def find_into(self, haystack, d_begin, d_end, d_number, capacity=None, delimiter=b"\n", stream=None):
        """ss_find_fields_device into the caller's 8-byte device tensors (each may be None; all three with capacity 0); returns the
        total."""
        ptr, length, t = DynamicHipSearcher._device_haystack(haystack)
        given = [x for x in (d_begin, d_end, d_number) if x is not None]
        if capacity is None:
            capacity = min(x.numel() for x in given) if given else 0
        total = _u64(0)
        with _on_device_of(t):
            st = stream if stream is not None else _current_stream_handle()
            p = [x.data_ptr() if x is not None else None for x in (d_begin, d_end, d_number)]
            _check(self._L.ss_find_fields_device(self._h, ptr, length, _delimiter_byte(delimiter), st, p[0], p[1], p[2], int(capacity),
                                                 ctypes.byref(total)), self._L)
        return total.value

    def find(self, haystack, delimiter=b"\n", capacity=None, stream=None):
        """(begin, end, number) int64 device tensors: the first ``capacity`` (default: all, counted first) records, ascending."""
        import torch
        ptr, length, t = DynamicHipSearcher._device_haystack(haystack)
        dev = t.device if t is not None else torch.device("cuda", torch.cuda.current_device())
        hay = t if t is not None else (ptr, length)
        if capacity is None:
            sel, tot = self.count(hay, delimiter, stream)
            capacity = tot if self.keep_short else sel
        out = torch.empty((3, max(int(capacity), 1)), dtype=torch.int64, device=dev)
        p = [out[k] if capacity else None for k in range(3)]
        total = self.find_into(hay, p[0], p[1], p[2], int(capacity), delimiter, stream)
        k = min(int(capacity), total)
        return out[0, :k], out[1, :k], out[2, :k]

    def cut(self, haystack, terminator=b"\n", delimiter=b"\n", stream=None):
        """uint8 device tensor: the selected fields of every record, each followed by ``terminator`` (None: none) - ``find``
        followed by ``ss.gather_ranges``: what ``cut -f`` prints."""
        ptr, length, t = DynamicHipSearcher._device_haystack(haystack)
        hay = t if t is not None else (ptr, length)
        begin, end, _ = self.find(hay, delimiter, None, stream)
        return _format(self._L, hay, begin, end, None, None, terminator, 0, stream, gather=True)

    def close(self):
        h, self._h = getattr(self, "_h", None), None
        L = getattr(self, "_L", None)
        if h and L is not None and _lib is not None:
            L.ss_fields_free(h)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# The grouping calls (include/sliceslice_hip_groups.h): functions of the module, since no handle owns them.
_GROUPS_ROWS = 1 << 16      # rows RunPattern.groups and group_lines make room for before they know the number of groups


def _groups_flags(ignore_case, weak_hash=False):
    return (SS_GROUPS_NOCASE if ignore_case else 0) | (SS_GROUPS_WEAK_HASH if weak_hash else 0)


def groups_scratch_bytes(n):
    """int: the temporary device memory a grouping call over ``n`` ranges takes (ss_groups_scratch_bytes; the run and the line
    form take 16 bytes per range more).  Host only; inside ``with ss.groups_build():``."""
    L = _feature_lib(lib(), "groups")
    n = int(n)
    if not 0 <= n <= _U64_MAX:
        raise ValueError("n is a number of ranges, 0 .. 2^64 - 1, got %d" % n)
    out = _u64(0)
    _check(L.ss_groups_scratch_bytes(n, ctypes.byref(out)), L)
    return int(out.value)


def group_ranges_into(haystack, begin, end, d_first, d_count, d_group=None, capacity=None, ignore_case=False, stream=None, weak_hash=False):
    """ss_group_ranges_device into the caller's 8-byte device tensors (each may be None; capacity: default the shorter of
    ``d_first`` and ``d_count``, 0 where both are None; ``d_group`` holds one entry per range); returns the number of groups.
    Inside ``with ss.groups_build():``."""
    import torch
    L = _feature_lib(lib(), "groups")
    ptr, length, t = DynamicHipSearcher._device_haystack(haystack)
    dev = t.device if t is not None else (begin.device if _is_tensor(begin) and begin.is_cuda else torch.device("cuda", torch.cuda.current_device()))
    given = [x for x in (d_first, d_count) if x is not None]
    if capacity is None:
        capacity = min(x.numel() for x in given) if given else 0
    groups = _u64(0)
    with _on_device_of(t if t is not None else begin):
        b, e = _device_numbers(begin, dev).reshape(-1), _device_numbers(end, dev).reshape(-1)
        if b.numel() != e.numel():
            raise ValueError("%d begins and %d ends" % (b.numel(), e.numel()))
        if d_group is not None and d_group.numel() < b.numel():
            raise ValueError("d_group holds one entry per range: %d, got %d" % (b.numel(), d_group.numel()))
        st = stream if stream is not None else _current_stream_handle()
        p = [x.data_ptr() if x is not None and x.numel() else None for x in (b, e, d_first, d_count, d_group)]
        _check(L.ss_group_ranges_device(ptr, length, p[0], p[1], b.numel(), _groups_flags(ignore_case, weak_hash), st, p[2], p[3], int(capacity),
                                        p[4], ctypes.byref(groups)), L)
    return groups.value


def group_ranges(haystack, begin, end, ignore_case=False, capacity=None, want_group=False, stream=None, weak_hash=False):
    """The ranges [begin[k], end[k]) of ``haystack`` - sequences, arrays or device tensors; they may overlap, repeat and descend
    and are clamped to the haystack - grouped by their bytes: ``(first, count)`` int64 device tensors with one row per distinct key
    in first-occurrence order (``first[j]`` is the smallest k of group j, ``count[j]`` its members: a ``collections.Counter`` filled
    in input order), the first ``capacity`` rows (default: all); ``want_group``: and ``group``, the j of every range
    (ss_group_ranges_device).  ``ignore_case`` folds ASCII letters before keys are compared.  Inside ``with ss.groups_build():``."""
    import torch
    _feature_lib(lib(), "groups")
    ptr, length, t = DynamicHipSearcher._device_haystack(haystack)
    dev = t.device if t is not None else (begin.device if _is_tensor(begin) and begin.is_cuda else torch.device("cuda", torch.cuda.current_device()))
    hay = t if t is not None else (ptr, length)
    b, e = _device_numbers(begin, dev).reshape(-1), _device_numbers(end, dev).reshape(-1)
    group = torch.empty(max(b.numel(), 1), dtype=torch.int64, device=dev)[:b.numel()] if want_group else None
    if capacity is None:
        # all rows: there are at most n of them, and one call fills them
        capacity = b.numel()
    out = torch.empty((2, max(int(capacity), 1)), dtype=torch.int64, device=dev)
    total = group_ranges_into(hay, b, e, out[0] if capacity else None, out[1] if capacity else None, group, int(capacity), ignore_case, stream,
                              weak_hash)
    k = min(int(capacity), total)
    return (out[0, :k], out[1, :k], group) if want_group else (out[0, :k], out[1, :k])


def group_lines_into(haystack, d_begin, d_end, d_number, d_count, capacity=None, delimiter=b"\n", ignore_case=False, stream=None, weak_hash=False):
    """ss_group_lines_device into the caller's 8-byte device tensors (each may be None); returns ``(groups, lines)``."""
    L = _feature_lib(lib(), "groups")
    ptr, length, t = DynamicHipSearcher._device_haystack(haystack)
    given = [x for x in (d_begin, d_end, d_number, d_count) if x is not None]
    if capacity is None:
        capacity = min(x.numel() for x in given) if given else 0
    groups, lines = _u64(0), _u64(0)
    with _on_device_of(t):
        st = stream if stream is not None else _current_stream_handle()
        p = [x.data_ptr() if x is not None and x.numel() else None for x in (d_begin, d_end, d_number, d_count)]
        _check(L.ss_group_lines_device(ptr, length, _delimiter_byte(delimiter), _groups_flags(ignore_case, weak_hash), st, p[0], p[1], p[2], p[3],
                                       int(capacity), ctypes.byref(groups), ctypes.byref(lines)), L)
    return groups.value, lines.value


def group_lines(haystack, delimiter=b"\n", ignore_case=False, stream=None, weak_hash=False):
    """(begin, end, number, count) int64 device tensors, one row per DISTINCT line of ``haystack`` in first-occurrence order: the
    record and the number of the first line with those bytes (the delimiter is no part of them; empty lines are lines) and how many
    there are - ``sort | uniq -c`` before the sort, ``awk '!seen[$0]++'`` (ss_group_lines_device with room for _GROUPS_ROWS rows;
    where there are more the WHOLE call is repeated, sized - ``group_lines_into`` with room for every row does it once).  Inside ``with ss.groups_build():``."""
    import torch
    _feature_lib(lib(), "groups")
    ptr, length, t = DynamicHipSearcher._device_haystack(haystack)
    dev = t.device if t is not None else torch.device("cuda", torch.cuda.current_device())
    hay = t if t is not None else (ptr, length)
    out = torch.empty((4, _GROUPS_ROWS), dtype=torch.int64, device=dev)
    total, _ = group_lines_into(hay, out[0], out[1], out[2], out[3], _GROUPS_ROWS, delimiter, ignore_case, stream, weak_hash)
    if total > _GROUPS_ROWS:
        out = torch.empty((4, total), dtype=torch.int64, device=dev)
        again, _ = group_lines_into(hay, out[0], out[1], out[2], out[3], total, delimiter, ignore_case, stream, weak_hash)
        total = min(total, again)
    return out[0, :total], out[1, :total], out[2, :total], out[3, :total]


class DynamicHipSearcher:
    """GPU counterpart of ``sliceslice::x86::DynamicAvx2Searcher`` (src/x86.rs:405-525)."""

    def __init__(self, needle, position=None, nocase=False):
        nb = needle.astype(np.uint8).tobytes() if isinstance(needle, np.ndarray) else bytes(needle)
        k, addr, n = _host_view(nb)
        self._h = ctypes.c_void_p()
        self._needle = nb
        L = self._L = lib()                 # the build this searcher belongs to (see tuning_build)
        if nocase:
            _check(_feature_lib(L, "nocase").ss_searcher_new_nocase(addr, n, ctypes.byref(self._h)), L)
            self._needle = fold_ascii(nb)   # (the library's copy is the folded one)
        elif position is None:
            _check(L.ss_searcher_new(addr, n, ctypes.byref(self._h)), L)
        else:
            _check(L.ss_searcher_with_position(addr, n, position % (1 << 64), ctypes.byref(self._h)), L)

    def _ck(self, rc):
        _check(rc, self._L)

    # -- reference-shaped constructors ---------------------------------------------------------------
    @classmethod
    def new(cls, needle):
        return cls(needle)

    @classmethod
    def with_position(cls, needle, position):
        return cls(needle, position)

    @classmethod
    def new_nocase(cls, needle):
        """ss_searcher_new_nocase (inside ``with ss.nocase_build():``): an ordinary searcher for ``fold_ascii(needle)`` - what the
        ``ignore_case=True`` forms of count / find_all / count_lines / find_lines take."""
        return cls(needle, nocase=True)

    @property
    def needle(self):
        return self._needle

    @property
    def position(self):
        n, pos = _sz(0), _sz(0)
        self._ck(self._L.ss_searcher_info(self._h, ctypes.byref(n), ctypes.byref(pos)))
        return pos.value

    # -- the hot path ------------------------------------------------------------------------------------
    def search_in(self, haystack, stream=None):
        """bool: does the needle occur in ``haystack``?  (DynamicAvx2Searcher::search_in)"""
        found = ctypes.c_int(0)
        if _is_tensor(haystack):
            if not haystack.is_cuda:
                return self.search_in(haystack.numpy())
            if haystack.dtype.itemsize != 1 or not haystack.is_contiguous():
                raise TypeError("device haystack must be a contiguous 1-byte tensor")
            with _on_device_of(haystack):
                st = stream if stream is not None else _current_stream_handle()
                self._ck(self._L.ss_search_device(self._h, haystack.data_ptr(), haystack.numel(), st, ctypes.byref(found)))
        elif isinstance(haystack, tuple):
            ptr, length = haystack
            st = stream if stream is not None else _current_stream_handle()
            self._ck(self._L.ss_search_device(self._h, ptr, length, st, ctypes.byref(found)))
        else:
            k, addr, n = _host_view(haystack)
            self._ck(self._L.ss_search_host(self._h, addr, n, ctypes.byref(found)))
        return bool(found.value)

    inlined_search_in = search_in       # src/x86.rs:498

    def find(self, haystack, stream=None):
        """Offset of the leftmost occurrence or None (row f1; the shape of tests/i386.rs:6-10
        `find_subsequence` and of the competitors in bench/benches/i386.rs).  Device tensors /
        (pointer, length) pairs use ss_find_device, host buffers ss_find_host."""
        pos = _u64(0)
        if isinstance(haystack, tuple) or (_is_tensor(haystack) and haystack.is_cuda):
            ptr, length = haystack if isinstance(haystack, tuple) else (haystack.data_ptr(), haystack.numel())
            with _on_device_of(haystack):
                st = stream if stream is not None else _current_stream_handle()
                self._ck(self._L.ss_find_device(self._h, ptr, length, st, ctypes.byref(pos)))
        else:
            if _is_tensor(haystack):
                haystack = haystack.numpy()
            k, addr, n = _host_view(haystack)
            self._ck(self._L.ss_find_host(self._h, addr, n, ctypes.byref(pos)))
        return None if pos.value == (1 << 64) - 1 else pos.value

    def find_async(self, haystack, d_best, base_offset=0, stream=None):
        """Enqueue only: atomicMin base_offset + offset into the uint64 device tensor d_best (init: all ones)."""
        with _on_device_of(haystack):
            st = stream if stream is not None else _current_stream_handle()
            self._ck(self._L.ss_find_device_async(self._h, haystack.data_ptr(), haystack.numel(), base_offset, st,
                                              d_best.data_ptr()))

    def search_in_async(self, haystack, d_flag, stream=None):
        """Enqueue only: OR the result into the int32 device tensor ``d_flag`` (caller-zeroed)."""
        with _on_device_of(haystack):
            st = stream if stream is not None else _current_stream_handle()
            self._ck(self._L.ss_search_device_async(self._h, haystack.data_ptr(), haystack.numel(), st, d_flag.data_ptr()))

    # -- every occurrence (libsliceslice_hip_matches.so: searchers made inside `with ss.matches_build():`) ----------------
    @staticmethod
    def _device_haystack(haystack):
        """(pointer, length, device tensor) of a haystack: device tensors as they are, host bytes uploaded to the current device."""
        if isinstance(haystack, tuple):
            return haystack[0], haystack[1], None
        import torch
        if not _is_tensor(haystack):
            haystack = torch.from_numpy(np.frombuffer(bytes(haystack), dtype=np.uint8).copy())
        if not haystack.is_cuda:
            haystack = haystack.contiguous().view(torch.uint8).cuda()
        if haystack.dtype.itemsize != 1 or not haystack.is_contiguous():
            raise TypeError("device haystack must be a contiguous 1-byte tensor")
        return haystack.data_ptr(), haystack.numel(), haystack

    def count(self, haystack, stream=None, ignore_case=False, whole_word=False):
        """int: the number of (overlapping) occurrences of the needle in ``haystack`` (ss_count_device).  Empty needle: len + 1.
        ignore_case=True (here and in the seven methods below; searchers made inside ``with ss.nocase_build():`` from a needle
        without upper-case bytes - ``new_nocase`` folds one): haystack letters match in either case (ss_count_nocase_device).
        whole_word=True (likewise; searchers made inside ``with ss.bounded_build():``, a non-empty needle): only occurrences whose
        two neighbour bytes are absent or no word bytes (``is_word_byte``) - ``grep -w`` (ss_count_bounded_device).  The four line
        methods also take a delimiter for a neighbour, and whole_line=True (``grep -x``): neighbours absent or the delimiter."""
        fn = _scan_fn(self._L, "ss_count_device", ignore_case, whole_word)
        ptr, length, t = self._device_haystack(haystack)
        c = _u64(0)
        with _on_device_of(t):
            st = stream if stream is not None else _current_stream_handle()
            self._ck(fn(self._h, ptr, length, st, ctypes.byref(c)))
        return c.value

    def count_async(self, haystack, d_count, stream=None, ignore_case=False, whole_word=False):
        """Enqueue only (ss_count_device_async): the count lands in the 8-byte device tensor ``d_count`` (overwritten)."""
        fn = _scan_fn(self._L, "ss_count_device_async", ignore_case, whole_word)
        with _on_device_of(haystack):
            st = stream if stream is not None else _current_stream_handle()
            self._ck(fn(self._h, haystack.data_ptr(), haystack.numel(), st, d_count.data_ptr()))

    def find_all(self, haystack, capacity=None, stream=None, ignore_case=False, whole_word=False):
        """int64 tensor on the haystack's device: the offsets of every (overlapping) occurrence in ascending order
        (ss_find_all_device).  capacity=None: counted first, then exactly that many; else the leftmost ``capacity`` of them."""
        import torch
        count_fn, find_fn = _scan_fn(self._L, "ss_count_device", ignore_case, whole_word), _scan_fn(self._L, "ss_find_all_device", ignore_case, whole_word)
        ptr, length, t = self._device_haystack(haystack)
        dev = t.device if t is not None else torch.device("cuda", torch.cuda.current_device())
        total = _u64(0)
        with _on_device_of(t):
            st = stream if stream is not None else _current_stream_handle()
            if capacity is None:
                self._ck(count_fn(self._h, ptr, length, st, ctypes.byref(total)))
                capacity = total.value
            out = torch.empty(max(int(capacity), 1), dtype=torch.int64, device=dev)
            self._ck(find_fn(self._h, ptr, length, st, out.data_ptr() if capacity else None, int(capacity),
                             ctypes.byref(total)))
        return out[:min(int(capacity), total.value)]

    def find_all_into(self, haystack, d_offsets, stream=None, ignore_case=False, whole_word=False):
        """ss_find_all_device into a caller's 8-byte device tensor (capacity = its length); returns the total count."""
        fn = _scan_fn(self._L, "ss_find_all_device", ignore_case, whole_word)
        ptr, length, t = self._device_haystack(haystack)
        total = _u64(0)
        with _on_device_of(t):
            st = stream if stream is not None else _current_stream_handle()
            self._ck(fn(self._h, ptr, length, st, d_offsets.data_ptr() if d_offsets.numel() else None, d_offsets.numel(), ctypes.byref(total)))
        return total.value

    # -- the non-overlapping occurrences (libsliceslice_hip_disjoint.so: searchers made inside `with ss.disjoint_build():`) ------
    @staticmethod
    def _disjoint_how(ignore_case, whole_word):
        return (SS_BOUND_WORD if whole_word else 0) | (SS_BOUND_NOCASE if ignore_case else 0)

    def count_disjoint(self, haystack, stream=None, ignore_case=False, whole_word=False):
        """int: the number of NON-OVERLAPPING occurrences of the needle, taken greedily from the left - ``bytes.count``
        (ss_count_disjoint_device).  ignore_case / whole_word as in ``count``; the bounds test comes before the selection."""
        L = _feature_lib(self._L, "disjoint")
        ptr, length, t = self._device_haystack(haystack)
        c = _u64(0)
        with _on_device_of(t):
            st = stream if stream is not None else _current_stream_handle()
            self._ck(L.ss_count_disjoint_device(self._h, ptr, length, self._disjoint_how(ignore_case, whole_word), st, ctypes.byref(c)))
        return c.value

    def find_all_disjoint_into(self, haystack, d_offsets, stream=None, ignore_case=False, whole_word=False):
        """ss_find_all_disjoint_device into a caller's 8-byte device tensor (capacity = its length); returns the total count."""
        L = _feature_lib(self._L, "disjoint")
        ptr, length, t = self._device_haystack(haystack)
        total = _u64(0)
        with _on_device_of(t):
            st = stream if stream is not None else _current_stream_handle()
            self._ck(L.ss_find_all_disjoint_device(self._h, ptr, length, self._disjoint_how(ignore_case, whole_word), st,
                                                   d_offsets.data_ptr() if d_offsets.numel() else None, d_offsets.numel(), ctypes.byref(total)))
        return total.value

    def find_all_disjoint(self, haystack, capacity=None, stream=None, ignore_case=False, whole_word=False):
        """int64 tensor on the haystack's device: the offsets of the non-overlapping occurrences in ascending order - what
        ``grep -o -b`` prints (ss_find_all_disjoint_device).  capacity=None: counted first, then exactly that many; else the leftmost
        ``capacity`` of them."""
        import torch
        _feature_lib(self._L, "disjoint")
        ptr, length, t = self._device_haystack(haystack)
        dev = t.device if t is not None else torch.device("cuda", torch.cuda.current_device())
        hay = t if t is not None else (ptr, length)
        if capacity is None:
            capacity = self.count_disjoint(hay, stream, ignore_case, whole_word)
        out = torch.empty(max(int(capacity), 1), dtype=torch.int64, device=dev)
        total = self.find_all_disjoint_into(hay, out[:int(capacity)], stream, ignore_case, whole_word)
        return out[:min(int(capacity), total)]

    def replace(self, haystack, replacement, stream=None, ignore_case=False, whole_word=False):
        """uint8 tensor on the haystack's device: the haystack with every non-overlapping occurrence of the needle replaced by
        ``replacement`` (host bytes, may be empty) - ``bytes.replace`` (ss_replace_device; sized with the count first)."""
        import torch
        L = _feature_lib(self._L, "disjoint")
        ptr, length, t = self._device_haystack(haystack)
        dev = t.device if t is not None else torch.device("cuda", torch.cuda.current_device())
        rep = bytes(replacement)
        keep, addr, rn = _host_view(rep)
        how = self._disjoint_how(ignore_case, whole_word)
        out_len, c = _u64(0), _u64(0)
        with _on_device_of(t):
            st = stream if stream is not None else _current_stream_handle()
            self._ck(L.ss_replace_device(self._h, ptr, length, how, addr, rn, st, None, 0, ctypes.byref(out_len), ctypes.byref(c)))
            out = torch.empty(max(out_len.value, 1), dtype=torch.uint8, device=dev)
            if out_len.value:
                self._ck(L.ss_replace_device(self._h, ptr, length, how, addr, rn, st, out.data_ptr(), out_len.value, ctypes.byref(out_len), ctypes.byref(c)))
        return out[:min(out_len.value, out.numel() if out_len.value else 0)]

    # -- the lines that contain the needle (libsliceslice_hip_lines.so: searchers made inside `with ss.lines_build():`) ------
    def count_lines(self, haystack, delimiter=b"\n", stream=None, ignore_case=False, whole_word=False, whole_line=False):
        """int: the number of lines of ``haystack`` (cut at every ``delimiter`` byte) that hold at least one occurrence of the
        needle - what ``grep -c`` prints (ss_count_lines_device).  Empty needle: the number of lines.  ignore_case=True folds the
        haystack's letters, never the delimiter."""
        return _count_lines(self, False, haystack, delimiter, stream, ignore_case, whole_word, whole_line)

    def count_lines_async(self, haystack, d_count, delimiter=b"\n", stream=None, ignore_case=False, whole_word=False, whole_line=False):
        """Enqueue only (ss_count_lines_device_async): the count lands in the 8-byte device tensor ``d_count`` (overwritten)."""
        return _count_lines_async(self, False, haystack, d_count, delimiter, stream, ignore_case, whole_word, whole_line)

    def find_lines(self, haystack, delimiter=b"\n", capacity=None, stream=None, ignore_case=False, whole_word=False, whole_line=False):
        """(begin, end, number): three int64 tensors on the haystack's device, one entry per matching line in ascending order - the
        offset of its first byte, the offset of the delimiter that closes it (len for a last line without one) and its 1-based
        line number (ss_find_lines_device).  capacity=None: counted first (ss_count_lines_device: one more pass over the haystack, as
        ``find_all`` does), then exactly that many; with a capacity the haystack is read at most twice and the leftmost ``capacity``
        records come back."""
        return _find_lines(self, False, haystack, delimiter, capacity, stream, ignore_case, whole_word, whole_line)

    def find_lines_into(self, haystack, d_begin, d_end, d_number, capacity, delimiter=b"\n", stream=None, ignore_case=False, whole_word=False, whole_line=False):
        """ss_find_lines_device into the caller's 8-byte device tensors (each may be None: not wanted); returns the total count."""
        return _find_lines_into(self, False, haystack, d_begin, d_end, d_number, capacity, delimiter, stream, ignore_case, whole_word, whole_line)

    # -- the lines that do NOT hold it (libsliceslice_hip_inverted.so: searchers made inside `with ss.inverted_build():`) ----
    # Methods of their own and not a keyword `invert` of the four above: tests/test_bounded_cpu.py pins the last parameters of those.
    def count_lines_inverted(self, haystack, delimiter=b"\n", stream=None, ignore_case=False, whole_word=False, whole_line=False):
        """int: the number of lines that ``count_lines`` with the same arguments does NOT count - ``grep -v -c``
        (ss_count_lines_inverted_device).  Together the two are the number of lines.  Empty needle: 0; a needle longer than the
        haystack or one that holds the delimiter: every line."""
        return _count_lines(self, True, haystack, delimiter, stream, ignore_case, whole_word, whole_line)

    def count_lines_inverted_async(self, haystack, d_count, delimiter=b"\n", stream=None, ignore_case=False, whole_word=False, whole_line=False):
        """Enqueue only (ss_count_lines_inverted_device_async): the count lands in the 8-byte device tensor ``d_count``."""
        return _count_lines_async(self, True, haystack, d_count, delimiter, stream, ignore_case, whole_word, whole_line)

    def find_lines_inverted(self, haystack, delimiter=b"\n", capacity=None, stream=None, ignore_case=False, whole_word=False, whole_line=False):
        """(begin, end, number) of the lines that ``find_lines`` with the same arguments does NOT return - ``grep -v -n``
        (ss_find_lines_inverted_device).  capacity=None: sized from the inverted count."""
        return _find_lines(self, True, haystack, delimiter, capacity, stream, ignore_case, whole_word, whole_line)

    def find_lines_inverted_into(self, haystack, d_begin, d_end, d_number, capacity, delimiter=b"\n", stream=None, ignore_case=False, whole_word=False, whole_line=False):
        """ss_find_lines_inverted_device into the caller's 8-byte device tensors (each may be None); returns the total count."""
        return _find_lines_into(self, True, haystack, d_begin, d_end, d_number, capacity, delimiter, stream, ignore_case, whole_word, whole_line)

    # -- with their context lines (libsliceslice_hip_context.so: searchers made inside `with ss.context_build():`) ------------
    def find_lines_context(self, haystack, before=0, after=0, delimiter=b"\n", capacity=None, stream=None,
                           ignore_case=False, whole_word=False, whole_line=False, invert=False):
        """(begin, end, number, kind): the records of the selected lines AND of the ``before`` lines in front of and the ``after``
        lines behind each of them, every line once, ascending - ``grep -B before -A after -n`` (ss_find_lines_context_device).
        kind (uint8) is 1 for a selected line and 0 for a context line; ``--`` stands wherever two consecutive numbers differ by
        more than one.  invert=True: the model is ``find_lines_inverted``.  capacity=None: counted first, then sized exactly."""
        return _find_lines_context(self, haystack, before, after, delimiter, capacity, stream, ignore_case, whole_word, whole_line, invert)

    def find_lines_context_into(self, haystack, d_begin, d_end, d_number, d_kind, capacity, before=0, after=0, delimiter=b"\n", stream=None,
                                ignore_case=False, whole_word=False, whole_line=False, invert=False):
        """ss_find_lines_context_device into the caller's device tensors (8-byte x3, 1-byte kind; each may be None); returns
        (total, selected): the size of the output and the number of selected lines."""
        return _find_lines_context_into(self, haystack, d_begin, d_end, d_number, d_kind, capacity, before, after, delimiter, stream,
                                        ignore_case, whole_word, whole_line, invert)

    def lines_around(self, haystack, numbers, before=0, after=0, delimiter=b"\n", capacity=None, stream=None):
        """(begin, end, number, kind) for the 1-based, strictly ascending line ``numbers`` (a sequence or a 64-bit tensor) and their
        context lines (ss_lines_around_device; the needle is not looked at).  before = after = 0: the records of the listed lines."""
        return _lines_around(self, haystack, numbers, before, after, delimiter, capacity, stream)

    def lines_around_into(self, haystack, numbers, d_begin, d_end, d_number, d_kind, capacity, before=0, after=0, delimiter=b"\n", stream=None):
        """ss_lines_around_device into the caller's device tensors (each may be None); returns the size of the output."""
        return _lines_around_into(self, haystack, numbers, d_begin, d_end, d_number, d_kind, capacity, before, after, delimiter, stream)

    # -- grep's output (libsliceslice_hip_output.so: searchers made inside `with ss.output_build():`) -----------------------------
    def grep(self, haystack, before=0, after=0, delimiter=b"\n", line_numbers=False, stream=None, ignore_case=False, whole_word=False,
             whole_line=False, invert=False):
        """uint8 tensor on the haystack's device: what ``grep -F needle`` writes to stdout - the selected lines and their ``before`` /
        ``after`` context lines, each closed by the delimiter, with ``number:`` / ``number-`` in front where ``line_numbers`` is
        set and ``--`` between groups exactly when ``before`` or ``after`` is non-zero, as in grep (ss_grep_lines_device: sized with
        a first call, then written).  The flags are ``find_lines_context``'s."""
        import torch
        L = _feature_lib(self._L, "output")
        ptr, length, t = self._device_haystack(haystack)
        dev = t.device if t is not None else torch.device("cuda", torch.cuda.current_device())
        flags = (SS_OUTPUT_NUMBER if line_numbers else 0) | (SS_OUTPUT_SEPARATOR if before or after else 0)
        how, d = _context_how(ignore_case, whole_word, whole_line, invert), _delimiter_byte(delimiter)
        b, a = _context_amount(before, "before"), _context_amount(after, "after")
        out_len, lines, selected = _u64(0), _u64(0), _u64(0)
        with _on_device_of(t):
            st = stream if stream is not None else _current_stream_handle()
            self._ck(L.ss_grep_lines_device(self._h, ptr, length, d, how, b, a, flags, st, None, 0, ctypes.byref(out_len), ctypes.byref(lines),
                                            ctypes.byref(selected)))
            out = torch.empty(max(out_len.value, 1), dtype=torch.uint8, device=dev)
            if out_len.value:
                self._ck(L.ss_grep_lines_device(self._h, ptr, length, d, how, b, a, flags, st, out.data_ptr(), out_len.value, ctypes.byref(out_len),
                                                ctypes.byref(lines), ctypes.byref(selected)))
        return out[:min(out_len.value, out.numel() if out_len.value else 0)]

    # -- tuning / measurement hooks ------------------------------------------------------------------
    @property
    def filter(self):
        """(first, second): indices of the first two needle bytes the filter tests."""
        return self.filter3[:2]

    @property
    def filter3(self):
        """(first, second, third): the bytes of the first-phase filter (third == second: a two-byte filter)."""
        a, b, c = _sz(0), _sz(0), _sz(0)
        self._ck(self._L.ss_searcher_filter3(self._h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)))
        return a.value, b.value, c.value

    def set_filter(self, first, second, third=None):
        """ss_searcher_set_filter3; third=None: a plain two-byte filter (third == second)."""
        self._ck(self._L.ss_searcher_set_filter3(self._h, first, second, second if third is None else third))

    def set_timing(self, on=True):
        self._ck(self._L.ss_searcher_set_timing(self._h, int(on)))

    def last_kernel_ms(self):
        ms = ctypes.c_float(0)
        self._ck(self._L.ss_searcher_last_kernel_ms(self._h, ctypes.byref(ms)))
        return ms.value

    def set_variant(self, variant):
        """Tuning builds only (ss_searcher_set_variant); 0 - the automatic choice - is accepted by every build."""
        if int(variant) != 0 or getattr(self._L, "has_hooks", False):
            self._ck(_feature_lib(self._L, "hooks").ss_searcher_set_variant(self._h, int(variant)))

    def set_grid(self, blocks):
        if int(blocks) != 0 or getattr(self._L, "has_hooks", False):
            self._ck(_feature_lib(self._L, "hooks").ss_searcher_set_grid(self._h, int(blocks)))

    def last_launch(self):
        """(workgroups per CU, workgroups in the grid) of the latest scan enqueued through this searcher on the current device."""
        w, g = ctypes.c_int(0), ctypes.c_uint(0)
        self._ck(self._L.ss_searcher_last_launch(self._h, ctypes.byref(w), ctypes.byref(g)))
        return w.value, g.value

    def device_triple(self):
        """The three first-phase bytes the device tests by default (ss_searcher_tuning_state.own): the searcher's triple, with the third byte
        the library adds to a plain pair."""
        st = TuningState()
        self._ck(self._L.ss_searcher_tuning_state(self._h, None, 0, ctypes.byref(st)))
        return tuple(int(x) for x in st.own)

    def tuning_state(self, haystack):
        """ss_searcher_tuning_state as a dict: what this handle has learnt about `haystack` (a device tensor) and goes by."""
        st = TuningState()
        self._ck(self._L.ss_searcher_tuning_state(self._h, haystack.data_ptr(), haystack.numel(), ctypes.byref(st)))
        return st.as_dict()

    def census_stats(self, haystack):
        """Hooks builds: the census's per-position match counts {pair_match, triple_match, pair_lanes, triple_lanes}, or None."""
        c = (ctypes.c_uint32 * 131)()
        have = ctypes.c_int(0)
        self._ck(_feature_lib(self._L, "hooks").ss_debug_census_stats(self._h, haystack.data_ptr(), haystack.numel(), c, ctypes.byref(have)))
        if not have.value:
            return None
        self.stats_roles = have.value - 1                   # the slot the pair counts were gathered for
        return {"pair_match": list(c[:64]), "triple_match": list(c[64:128]), "pair_lanes": int(c[128]), "triple_lanes": int(c[129]), "deep_lanes": int(c[130])}

    def census(self, haystack):
        """Hooks builds: the candidate census of (this searcher, haystack) as a dict, or None when its counts are not in."""
        c = (ctypes.c_uint32 * 11)()
        ptr, n = haystack.data_ptr(), haystack.numel()
        self._ck(_feature_lib(self._L, "hooks").ss_debug_census(self._h, ptr, n, c))
        self.last_mode = int(c[5])                          # kernel family of the latest launch (0, 2 or 3)
        self.device_filter = (int(c[6]), int(c[7]), int(c[8]))      # the bytes the device tests on this haystack
        self.triple_state, self.triple_trials = int(c[9]), int(c[10])  # 0 undecided / 1 own / 2 from the histogram; trials so far
        if c[0] == 0:
            return None
        return {"tiles": c[0], "tiles3": c[1], "tiles2": c[2], "match_tiles": c[3], "lanes": c[4]}

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        L = getattr(self, "_L", None)
        if h and L is not None and _lib is not None:
            L.ss_searcher_free(h)


class HipSearcher(DynamicHipSearcher):
    """GPU counterpart of ``sliceslice::x86::Avx2Searcher`` (src/x86.rs:266-382): the searcher for needles of at
    least one byte - an EMPTY needle panics in the reference (`position = size.wrapping_sub(1)` fails
    `assert!(position < size)`, src/x86.rs:285-300; test `avx2_empty_needle`, src/x86.rs:545-549), where the dynamic
    searcher answers `true`.  Everything else is the dynamic searcher's behaviour."""

    def __init__(self, needle, position=None):
        nb = needle.astype(np.uint8).tobytes() if isinstance(needle, np.ndarray) else bytes(needle)
        if len(nb) == 0:
            raise PositionError(SS_ERR_POSITION, "Avx2Searcher contract: the needle must not be empty (src/x86.rs:300)")
        if position is not None and position >= len(nb):
            raise PositionError(SS_ERR_POSITION, "position %d out of range for a needle of %d bytes" % (position, len(nb)))
        super().__init__(nb, position)


class MemchrHipSearcher:
    """GPU counterpart of ``sliceslice::MemchrSearcher`` (src/lib.rs:119-142): one byte, `search_in` is false for an
    empty haystack."""

    def __init__(self, needle):
        b = int(needle)
        if not 0 <= b <= 255:
            raise ValueError("MemchrHipSearcher takes one byte (0..255)")
        self._inner = DynamicHipSearcher(bytes([b]))

    @classmethod
    def new(cls, needle):
        return cls(needle)

    def search_in(self, haystack, stream=None):
        return self._inner.search_in(haystack, stream)

    inlined_search_in = search_in

    def find(self, haystack, stream=None):
        return self._inner.find(haystack, stream)

    def count(self, haystack, stream=None, ignore_case=False, whole_word=False):
        return self._inner.count(haystack, stream, ignore_case, whole_word)

    def find_all(self, haystack, capacity=None, stream=None, ignore_case=False, whole_word=False):
        return self._inner.find_all(haystack, capacity, stream, ignore_case, whole_word)

    def count_lines(self, haystack, delimiter=b"\n", stream=None, ignore_case=False, whole_word=False, whole_line=False):
        return self._inner.count_lines(haystack, delimiter, stream, ignore_case, whole_word, whole_line)

    def count_lines_async(self, haystack, d_count, delimiter=b"\n", stream=None, ignore_case=False, whole_word=False, whole_line=False):
        return self._inner.count_lines_async(haystack, d_count, delimiter, stream, ignore_case, whole_word, whole_line)

    def find_lines(self, haystack, delimiter=b"\n", capacity=None, stream=None, ignore_case=False, whole_word=False, whole_line=False):
        return self._inner.find_lines(haystack, delimiter, capacity, stream, ignore_case, whole_word, whole_line)

    def find_lines_into(self, haystack, d_begin, d_end, d_number, capacity, delimiter=b"\n", stream=None, ignore_case=False, whole_word=False, whole_line=False):
        return self._inner.find_lines_into(haystack, d_begin, d_end, d_number, capacity, delimiter, stream, ignore_case, whole_word, whole_line)

    def count_lines_inverted(self, haystack, delimiter=b"\n", stream=None, ignore_case=False, whole_word=False, whole_line=False):
        return self._inner.count_lines_inverted(haystack, delimiter, stream, ignore_case, whole_word, whole_line)

    def count_lines_inverted_async(self, haystack, d_count, delimiter=b"\n", stream=None, ignore_case=False, whole_word=False, whole_line=False):
        return self._inner.count_lines_inverted_async(haystack, d_count, delimiter, stream, ignore_case, whole_word, whole_line)

    def find_lines_inverted(self, haystack, delimiter=b"\n", capacity=None, stream=None, ignore_case=False, whole_word=False, whole_line=False):
        return self._inner.find_lines_inverted(haystack, delimiter, capacity, stream, ignore_case, whole_word, whole_line)

    def find_lines_inverted_into(self, haystack, d_begin, d_end, d_number, capacity, delimiter=b"\n", stream=None, ignore_case=False, whole_word=False, whole_line=False):
        return self._inner.find_lines_inverted_into(haystack, d_begin, d_end, d_number, capacity, delimiter, stream, ignore_case, whole_word, whole_line)

    def find_lines_context(self, haystack, before=0, after=0, delimiter=b"\n", capacity=None, stream=None,
                           ignore_case=False, whole_word=False, whole_line=False, invert=False):
        return self._inner.find_lines_context(haystack, before, after, delimiter, capacity, stream, ignore_case, whole_word, whole_line, invert)

    def find_lines_context_into(self, haystack, d_begin, d_end, d_number, d_kind, capacity, before=0, after=0, delimiter=b"\n", stream=None,
                                ignore_case=False, whole_word=False, whole_line=False, invert=False):
        return self._inner.find_lines_context_into(haystack, d_begin, d_end, d_number, d_kind, capacity, before, after, delimiter, stream,
                                                   ignore_case, whole_word, whole_line, invert)

    def lines_around(self, haystack, numbers, before=0, after=0, delimiter=b"\n", capacity=None, stream=None):
        return self._inner.lines_around(haystack, numbers, before, after, delimiter, capacity, stream)

    def lines_around_into(self, haystack, numbers, d_begin, d_end, d_number, d_kind, capacity, before=0, after=0, delimiter=b"\n", stream=None):
        return self._inner.lines_around_into(haystack, numbers, d_begin, d_end, d_number, d_kind, capacity, before, after, delimiter, stream)

    def grep(self, haystack, before=0, after=0, delimiter=b"\n", line_numbers=False, stream=None, ignore_case=False, whole_word=False,
             whole_line=False, invert=False):
        return self._inner.grep(haystack, before, after, delimiter, line_numbers, stream, ignore_case, whole_word, whole_line, invert)


def shard_range(length, needle_len, nranks, rank):
    """Byte range [begin, end) of `rank`'s shard: S = ceil(len/G), n-1 bytes of overlap to the right."""
    b, e = _sz(0), _sz(0)
    _check(lib().ss_shard_range(length, needle_len, nranks, rank, ctypes.byref(b), ctypes.byref(e)))
    return b.value, e.value


class ShardedSearcher:
    """Range-sharded search over the GPUs of one node: one process per GPU, each holding its shard.

    ``search_in(shard)`` scans the local shard and combines the found flag with ONE all-reduce(MAX)
    (OR over {0,1}; RCCL has no OR).  Two transports:
      * ``backend="rccl"``  - native RCCL through the C ABI (ss_comm_*), all on one HIP stream;
      * ``backend="torch"`` - torch.distributed.all_reduce on the given process group (RCCL on GPUs,
        gloo on CPU - used by the CPU tests with an injected shard searcher).
    """

    def __init__(self, needle, position=None, group=None, backend="torch", local_search=None, local_find=None):
        import torch.distributed as dist
        self._dist = dist
        self.group = group
        self.rank = dist.get_rank(group)
        self.nranks = dist.get_world_size(group)
        self.needle = bytes(needle)
        self.backend = backend
        self._local_search = local_search
        self._local_find = local_find
        self._best = None
        self._searcher = None if (local_search is not None or local_find is not None) else \
            DynamicHipSearcher(needle, position)
        self._comm = None
        self._flag = None
        self._flag_next = 0
        self._L = self._searcher._L if self._searcher is not None else lib()
        if backend == "rccl":
            self._init_rccl()

    def shard_range(self, total_len):
        return shard_range(total_len, len(self.needle), self.nranks, self.rank)

    def _ck(self, rc):
        _check(rc, self._L)

    def fail_next_scans(self, count=1):
        """Hooks builds: the next `count` scans of this rank fail before they reach the device (ss_debug_fail_next_scans)."""
        self._ck(_feature_lib(self._L, "hooks").ss_debug_fail_next_scans(self._searcher._h, count))

    def _init_rccl(self):
        import torch
        uid = (ctypes.c_uint8 * 128)()
        box = [None]
        if self.rank == 0 and self._L.ss_comm_unique_id(uid) == 0:
            box = [bytes(uid)]
        self._dist.broadcast_object_list(box, src=0, group=self.group)     # None: rank 0 has no id to offer
        if box[0] is None:
            raise SlicesliceError(SS_ERR_RCCL, "rank 0 could not create an RCCL unique id" +
                                  (": " + self._L.ss_last_error().decode("utf-8", "replace") if self.rank == 0 else ""))
        uid = (ctypes.c_uint8 * 128).from_buffer_copy(box[0])
        comm = ctypes.c_void_p()
        # ncclCommInitRank is a collective: a rank on which it fails (or never returns) must not leave the others
        # behind in it, and all ranks must take the same road afterwards.  It runs on a worker thread with a time
        # limit (SLICESLICE_RCCL_INIT_TIMEOUT seconds, default 180); then the ranks agree - all-reduce(MIN) of "mine
        # worked" on the torch group - and either all keep their communicator or all raise.
        import threading
        result = {}
        dev = torch.cuda.current_device() if torch.cuda.is_available() else None

        def work():
            try:
                if dev is not None:
                    torch.cuda.set_device(dev)
                result["rc"] = self._L.ss_comm_init_rank(uid, self.nranks, self.rank, ctypes.byref(comm))
                result["err"] = self._L.ss_last_error().decode("utf-8", "replace") if result["rc"] else ""
            except Exception as e:                                   # pragma: no cover - ctypes / loader failures
                result["rc"], result["err"] = -1, repr(e)

        t = threading.Thread(target=work, daemon=True)
        t.start()
        t.join(float(os.environ.get("SLICESLICE_RCCL_INIT_TIMEOUT", "180")))
        mine = 1 if (not t.is_alive() and result.get("rc") == 0) else 0
        on_gpu = self._dist.get_backend(self.group) == "nccl"
        ok = torch.tensor([mine], dtype=torch.int32, device="cuda" if on_gpu else "cpu")
        self._dist.all_reduce(ok, op=self._dist.ReduceOp.MIN, group=self.group)
        if int(ok.item()) != 1:
            if mine:
                self._L.ss_comm_free(comm)
            why = "timed out" if t.is_alive() else (result.get("err") or "failed on another rank")
            raise SlicesliceError(SS_ERR_RCCL, "native RCCL communicator not built on every rank (this rank: %s)" % why)
        self._comm = comm
        torch.cuda.synchronize()

    def _peer_error(self):
        return SlicesliceError(SS_ERR_PEER, "another rank failed the local part of this sharded search; no answer")

    def search_in(self, shard, stream=None):
        """Collective-safe: a rank whose local part raises still takes part in the all-reduce (contributing "not found"
        and raising the second word of the flag pair), then re-raises; the other ranks raise SlicesliceError(SS_ERR_PEER)
        - nobody is left waiting in the collective."""
        import torch
        if self._local_search is not None:                       # CPU tests: injected shard searcher
            err = None
            try:
                f = 1 if self._local_search(shard) else 0
            except Exception as e:                                # noqa: BLE001 - re-raised behind the collective
                err, f = e, 0
            flag = torch.tensor([f, 1 if err is not None else 0], dtype=torch.int32)
            self._dist.all_reduce(flag, op=self._dist.ReduceOp.MAX, group=self.group)
            if err is not None:
                raise err
            if int(flag[1]):
                raise self._peer_error()
            return bool(flag[0])
        if self.backend == "rccl":
            found = ctypes.c_int(0)
            with _on_device_of(shard):
                st = stream if stream is not None else _current_stream_handle()
                self._ck(self._L.ss_search_sharded(self._searcher._h, shard.data_ptr(), shard.numel(), self._comm, st,
                                               ctypes.byref(found)))
            return bool(found.value)
        # torch transport: the scan, the flag housekeeping and the all-reduce must all be ordered on ONE stream -
        # torch's current stream.  A caller-supplied stream (object or raw handle) is made current for the duration.
        with _on_device_of(shard), self._as_current(stream):
            # a ring of pre-zeroed flag PAIRS {found, a rank failed}: one fresh pair per call, one zero_() launch per 256
            # calls instead of per call
            if self._flag is None or self._flag_next == self._flag.numel():
                if self._flag is None:
                    self._flag = torch.zeros(512, dtype=torch.int32, device=shard.device)
                else:
                    self._flag.zero_()
                self._flag_next = 0
            flag = self._flag[self._flag_next:self._flag_next + 2]
            self._flag_next += 2
            err = None
            try:
                self._searcher.search_in_async(shard, flag[0:1])
            except Exception as e:                                # noqa: BLE001 - re-raised behind the collective
                err = e
                flag[1:2].fill_(1)
            self._dist.all_reduce(flag, op=self._dist.ReduceOp.MAX, group=self.group)
            f, failed = flag.tolist()
            if err is not None:
                raise err
            if failed:
                raise self._peer_error()
            return bool(f)

    @staticmethod
    def _as_current(stream):
        import contextlib
        import torch
        if stream is None:
            return contextlib.nullcontext()
        if isinstance(stream, int):
            stream = torch.cuda.ExternalStream(stream)
        return torch.cuda.stream(stream)

    def find(self, shard, shard_begin, stream=None):
        """Global offset of the leftmost occurrence in the logical haystack, or None: every rank finds its
        local leftmost match (offset + shard_begin), ONE all-reduce(MIN) combines them."""
        import torch
        none = (1 << 63) - 1                                      # int64 stand-in for SS_NPOS in the reduce
        err = None
        if self._local_find is not None:                          # CPU tests: injected shard find
            try:
                p = self._local_find(shard)
            except Exception as e:                                # noqa: BLE001 - re-raised behind the collective
                err, p = e, None
            t = torch.tensor([none if p is None else p + shard_begin, -1 if err is not None else none], dtype=torch.int64)
        elif self.backend == "rccl":                              # native: ncclAllReduce(uint64 pair, ncclMin)
            pos = _u64(0)
            with _on_device_of(shard):
                st = stream if stream is not None else _current_stream_handle()
                self._ck(self._L.ss_find_sharded(self._searcher._h, shard.data_ptr(), shard.numel(), shard_begin, self._comm, st,
                                             ctypes.byref(pos)))
            return None if pos.value == (1 << 64) - 1 else pos.value
        else:
            with _on_device_of(shard), self._as_current(stream):   # everything ordered on one (the current) stream
                if self._best is None:
                    self._best = torch.empty(1, dtype=torch.int64, device=shard.device)
                self._best.fill_(-1)                               # all ones = SS_NPOS
                try:
                    self._searcher.find_async(shard, self._best, shard_begin)
                except Exception as e:                            # noqa: BLE001
                    err = e
                b = torch.where(self._best < 0, torch.full_like(self._best, none), self._best)
                t = torch.cat([b, torch.full_like(b, -1 if err is not None else none)])
                self._dist.all_reduce(t, op=self._dist.ReduceOp.MIN, group=self.group)
                v, status = (int(x) for x in t.tolist())
            if err is not None:
                raise err
            if status != none:
                raise self._peer_error()
            return None if v == none else v
        # second word of the pair: `none` unless a rank failed its local part (MIN brings the -1 to everybody)
        self._dist.all_reduce(t, op=self._dist.ReduceOp.MIN, group=self.group)
        v, status = (int(x) for x in t.tolist())
        if err is not None:
            raise err
        if status != none:
            raise self._peer_error()
        return None if v == none else v

    def rccl_ranks(self):
        """Number of ranks RCCL itself reports for the native communicator (ncclCommCount), or None."""
        if self._comm is None:
            return None
        n = ctypes.c_int(0)
        self._ck(self._L.ss_comm_count(self._comm, ctypes.byref(n)))
        return n.value

    def close(self):
        if self._comm is not None and _lib is not None:
            self._L.ss_comm_free(self._comm)
            self._comm = None


class NodeSearcher:
    """Range-sharded search over several GPUs from ONE process (ss_comm_init_all / ss_search_sharded_all):
    what a drop-in ``search_in(&self, haystack) -> bool`` (src/x86.rs:523) over the GPUs of a node calls - no
    launcher, no rendezvous.  ``shards`` is a list of uint8 tensors, shard g resident on device g of the set
    (ranges from ``shard_range``)."""

    COMBINE_RCCL, COMBINE_HOST = 0, 1
    ISSUE_THREADS, ISSUE_SERIAL = 0, 1

    def __init__(self, needle, position=None, devices=None, ndev=None):
        import torch
        if devices is None:
            devices = list(range(ndev if ndev is not None else torch.cuda.device_count()))
        self.devices = list(devices)
        arr = (ctypes.c_int * len(self.devices))(*self.devices)
        self._set = ctypes.c_void_p()
        L = self._L = lib()
        _check(L.ss_comm_init_all(len(self.devices), arr, ctypes.byref(self._set)), L)
        self._searcher = DynamicHipSearcher(needle, position)
        self.needle = bytes(needle)

    def set_combine(self, mode):
        self._ck(self._L.ss_comm_set_combine(self._set, mode))

    def set_issue(self, mode):
        """ISSUE_THREADS: one issue thread per device (the default from two devices up); ISSUE_SERIAL: the calling thread."""
        self._ck(self._L.ss_comm_set_issue(self._set, mode))

    def rccl_ranks(self):
        """ncclCommCount of every communicator of the set (they must agree), or None for a set without communicators."""
        n = ctypes.c_int(0)
        if self._L.ss_comm_set_count(self._set, ctypes.byref(n)) != 0:
            return None
        return n.value

    def last_kernel_ms(self):
        """Every device's scan-kernel time of the latest search (the searcher's timing must be on)."""
        ms = (ctypes.c_float * len(self.devices))()
        self._ck(self._L.ss_comm_set_last_kernel_ms(self._set, ms, len(self.devices)))
        return [float(x) for x in ms]

    def last_issue_us(self):
        """Host microseconds the latest search spent issuing (scans, collective, answer words, all of it)."""
        us = (ctypes.c_float * 4)()
        self._ck(self._L.ss_comm_set_last_issue_us(self._set, us))
        return [float(x) for x in us]

    def _ck(self, rc):
        _check(rc, self._L)

    def set_epoch(self, value):
        """Hooks builds: move the set's "found" epoch (ss_debug_set_comm_epoch) so that a test can cross the 2^31 wrap."""
        self._ck(_feature_lib(self._L, "hooks").ss_debug_set_comm_epoch(None, self._set, value))

    def shard_range(self, total_len, g):
        return shard_range(total_len, len(self.needle), len(self.devices), g)

    def _args(self, shards):
        G = len(self.devices)
        assert len(shards) == G
        for g, t in enumerate(shards):
            assert t.is_cuda and t.device.index == self.devices[g] and t.dtype.itemsize == 1 and t.is_contiguous()
        ptrs = (ctypes.c_void_p * G)(*[t.data_ptr() if t.numel() else None for t in shards])
        lens = (_sz * G)(*[t.numel() for t in shards])
        return ptrs, lens

    def search_in(self, shards):
        ptrs, lens = self._args(shards)
        found = ctypes.c_int(0)
        self._ck(self._L.ss_search_sharded_all(self._searcher._h, ptrs, lens, self._set, ctypes.byref(found)))
        return bool(found.value)

    def find(self, shards, begins):
        ptrs, lens = self._args(shards)
        b = (_u64 * len(begins))(*begins)
        pos = _u64(0)
        self._ck(self._L.ss_find_sharded_all(self._searcher._h, ptrs, lens, b, self._set, ctypes.byref(pos)))
        return None if pos.value == (1 << 64) - 1 else pos.value

    def close(self):
        if getattr(self, "_set", None) and _lib is not None:
            self._L.ss_comm_set_free(self._set)
            self._set = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class SearchService:
    """A resident search service on the current device (ss_service_*): a small kernel that stays on the GPU and takes one search
    at a time from a mailbox in device memory that the host writes through the PCIe BAR - no launch per search (5 us instead
    of 8.5-9.5; ``bind`` a haystack that does not change between searches).  ``search_in(searcher, haystack)`` has the semantics of
    ``searcher.search_in(haystack)`` for a device haystack whose bytes are COMPLETE (the service is not ordered behind pending
    stream work)."""

    def __init__(self, workgroups=0, lease_ms=0.0):
        self._h = ctypes.c_void_p()
        L = self._L = _feature_lib(lib(), "service")
        _check(L.ss_service_start(int(workgroups), float(lease_ms), ctypes.byref(self._h)), L)

    def _ck(self, rc):
        _check(rc, self._L)

    def search_in(self, searcher, haystack):
        found = ctypes.c_int(0)
        ptr, n = (haystack.data_ptr(), haystack.numel()) if hasattr(haystack, "data_ptr") else haystack
        assert searcher._L is self._L, "searcher and service come from different builds of the library"
        self._ck(self._L.ss_service_search(self._h, searcher._h, ptr if n else None, n, ctypes.byref(found)))
        return bool(found.value)

    def bind(self, haystack):
        """The caller vouches that this device range stays unchanged until ``unbind()`` / the next ``bind``: searches inside it
        skip the per-request cache acquire (all but the first, and those whose searcher was uploaded after it)."""
        ptr, n = (haystack.data_ptr(), haystack.numel()) if hasattr(haystack, "data_ptr") else haystack
        self._ck(self._L.ss_service_bind(self._h, ptr if n else None, n))

    def unbind(self):
        self._ck(self._L.ss_service_bind(self._h, None, 0))

    def counters(self):
        """(requests served, kernel launches, requests that skipped the acquire) - hooks builds (ss_service_counters)."""
        r, k, t = _u64(0), _u64(0), _u64(0)
        self._ck(_feature_lib(self._L, "hooks").ss_service_counters(self._h, ctypes.byref(r), ctypes.byref(k), ctypes.byref(t)))
        return r.value, k.value, t.value

    def stop(self):
        if getattr(self, "_h", None) and _lib is not None:
            self._L.ss_service_stop(self._h)
            self._h = None

    close = stop

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.stop()

    def __del__(self):
        try:
            self.stop()
        except Exception:
            pass


class BatchPlan:
    """Plan once, search many (ss_batch_plan_*): the per-problem set-up of ``search_batched`` / ``find_batched`` done once - the
    reference builds its 4,585 searchers once and times the searches (bench/benches/i386.rs:246-256).  ``run()`` is ONE kernel
    launch that also re-arms the outputs; it can be captured into a hipGraph.  Arguments as ``search_batched``; the tensors
    must stay alive (and their ranges / needle bytes unchanged) as long as the plan is used."""

    def __init__(self, haystacks, hay_off, needles, needle_off, position=None, find=False, stream=None, hay_ranges=None,
                 needle_ranges=None):
        hb, he, count = _ranges(hay_off, *(hay_ranges or (None, None)))
        nb, ne, ncount = _ranges(needle_off, *(needle_ranges or (None, None)))
        assert count == ncount
        self._keep = (haystacks, hay_off, needles, needle_off, position, hay_ranges, needle_ranges)
        self.count, self.find, self.device = count, bool(find), haystacks.device
        self._h = ctypes.c_void_p()
        L = self._L = lib()
        st = stream if stream is not None else _current_stream_handle()
        _check(L.ss_batch_plan_create(haystacks.data_ptr(), hb, he, needles.data_ptr(), nb, ne,
                                      position.data_ptr() if position is not None else None, count, int(self.find), st,
                                      ctypes.byref(self._h)), L)

    def run(self, out=None, stream=None):
        """Enqueues the search; returns the output tensor (int32 flags, or int64 offsets with -1 = absent for find plans)."""
        import torch
        if out is None:
            out = torch.empty(self.count, dtype=torch.int64 if self.find else torch.int32, device=self.device)
        st = stream if stream is not None else _current_stream_handle()
        _check(self._L.ss_batch_plan_run(self._h, st, out.data_ptr()), self._L)
        return out

    def filter_of(self, problem):
        """((first, second, third) indices in the needle, the packed bytes, slices that scan the problem) of one problem's
        descriptor - hooks builds (ss_debug_plan_filter)."""
        out = (ctypes.c_uint32 * 5)()
        _check(_feature_lib(self._L, "hooks").ss_debug_plan_filter(self._h, int(problem), out), self._L)
        return (out[0], out[1], out[2]), out[3], out[4]

    def layout(self):
        """{"two": the plan holds two layouts, "slices": (first, second), "found_last": problems found in the latest tallied run,
        "next_is_second": the next run takes the contiguous-runs layout} - hooks builds (ss_debug_plan_layout)."""
        out = (ctypes.c_uint32 * 5)()
        _check(_feature_lib(self._L, "hooks").ss_debug_plan_layout(self._h, out), self._L)
        return {"two": bool(out[0]), "slices": (out[1], out[2]), "found_last": out[3], "next_is_second": bool(out[4])}

    def cold_of(self, problem):
        """(schedule indices, schedule bytes, exact_len, bytes in front, the compare's 16 bytes) of one problem's ready-made cold
        part - hooks builds (ss_debug_plan_cold)."""
        out = (ctypes.c_uint32 * 14)()
        _check(_feature_lib(self._L, "hooks").ss_debug_plan_cold(self._h, int(problem), out), self._L)
        n = out[0]
        idx = b"".join(int(out[2 + t]).to_bytes(4, "little") for t in range(4))[:n]
        val = b"".join(int(out[6 + t]).to_bytes(4, "little") for t in range(4))[:n]
        tail = b"".join(int(out[10 + t]).to_bytes(4, "little") for t in range(4))
        return list(idx), val, out[1] & 0xFF, out[1] >> 8, tail

    def close(self):
        if getattr(self, "_h", None) and _lib is not None:
            self._L.ss_batch_plan_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def batch_classes(haystacks, hay_off=None, hay_ranges=None):
    """(state, classes) the library remembers for the UNPLANNED batch calls on these haystacks / ranges: state 0 unknown, 1 named
    once, 2 sampling in flight, 3 classes in (then a list of 256 rarity classes, 0 = rarest) - hooks builds (ss_debug_batch_classes)."""
    hb, _, count = _ranges(hay_off, *(hay_ranges or (None, None)))
    st, cls = ctypes.c_uint32(0), (ctypes.c_uint8 * 256)()
    L = lib()
    _check(_feature_lib(L, "hooks").ss_debug_batch_classes(haystacks.data_ptr(), hb, count, ctypes.byref(st), cls), L)
    return st.value, (list(cls) if st.value == 3 else None)


def _ranges(off, begin, end):
    """(begin_ptr, end_ptr, count) from either CSR offsets (count+1 int64) or explicit begin/end arrays."""
    if off is not None:
        return off.data_ptr(), off.data_ptr() + 8, off.numel() - 1
    return begin.data_ptr(), end.data_ptr(), begin.numel()


def search_batched(haystacks, hay_off, needles, needle_off, position=None, stream=None, hay_ranges=None,
                   needle_ranges=None, pairs=False):
    """One launch for many (needle_i, haystack_i) problems; all arguments are device tensors (uint8
    blobs; int64 CSR offsets of length count+1, or explicit (begin, end) tensor pairs via *_ranges, which
    may alias).  ``pairs=True`` uses the lane-per-problem kernel for tiny haystacks (ss_search_pairs).
    Returns an int32 device tensor of flags."""
    import torch
    hb, he, count = _ranges(hay_off, *(hay_ranges or (None, None)))
    nb, ne, ncount = _ranges(needle_off, *(needle_ranges or (None, None)))
    assert count == ncount
    found = torch.empty(count, dtype=torch.int32, device=haystacks.device)
    st = stream if stream is not None else _current_stream_handle()
    fn = lib().ss_search_pairs if pairs else lib().ss_search_batched
    _check(fn(haystacks.data_ptr(), hb, he, needles.data_ptr(), nb, ne,
              position.data_ptr() if position is not None else None, count, st, found.data_ptr()))
    return found


def find_batched(haystacks, hay_off, needles, needle_off, stream=None, hay_ranges=None, needle_ranges=None):
    """Leftmost offset of needle i in haystack i for many problems in one call (ss_find_batched); -1 where absent.  Arguments as
    search_batched.  Returns an int64 device tensor."""
    import torch
    hb, he, count = _ranges(hay_off, *(hay_ranges or (None, None)))
    nb, ne, ncount = _ranges(needle_off, *(needle_ranges or (None, None)))
    assert count == ncount
    pos = torch.empty(count, dtype=torch.int64, device=haystacks.device)
    st = stream if stream is not None else _current_stream_handle()
    _check(lib().ss_find_batched(haystacks.data_ptr(), hb, he, needles.data_ptr(), nb, ne, count, st, pos.data_ptr()))
    return pos                                      # SS_NPOS (all ones) reads as -1


def count_batched(haystacks, hay_off, needles, needle_off, stream=None, hay_ranges=None, needle_ranges=None):
    """(Overlapping) occurrences of needle i in haystack i for many problems in one call (ss_count_batched; inside
    ``with ss.matches_batched_build():``).  Arguments as search_batched.  Enqueue only; returns an int64 device tensor."""
    import torch
    L = _feature_lib(lib(), "matches_batched")
    hb, he, count = _ranges(hay_off, *(hay_ranges or (None, None)))
    nb, ne, ncount = _ranges(needle_off, *(needle_ranges or (None, None)))
    assert count == ncount
    counts = torch.empty(count, dtype=torch.int64, device=haystacks.device)
    st = stream if stream is not None else _current_stream_handle()
    _check(L.ss_count_batched(haystacks.data_ptr(), hb, he, needles.data_ptr(), nb, ne, count, st, counts.data_ptr()), L)
    return counts


def find_all_batched(haystacks, hay_off, needles, needle_off, stream=None, hay_ranges=None, needle_ranges=None, capacity=None):
    """Every (overlapping) occurrence of needle i in haystack i for many problems, in CSR form (ss_find_all_batched; inside
    ``with ss.matches_batched_build():``): ``(counts, row_begin, offsets)`` - int64 device tensors of count, count + 1 and
    min(total, capacity) entries; ``offsets[row_begin[i]:row_begin[i + 1]]`` are problem i's offsets relative to its own haystack,
    ascending (rows beyond ``capacity`` are cut).  capacity=None: counted first, then exactly that many.  Waits for the stream."""
    import torch
    L = _feature_lib(lib(), "matches_batched")
    hb, he, count = _ranges(hay_off, *(hay_ranges or (None, None)))
    nb, ne, ncount = _ranges(needle_off, *(needle_ranges or (None, None)))
    assert count == ncount
    dev = haystacks.device
    counts = torch.empty(count, dtype=torch.int64, device=dev)
    rows = torch.empty(count + 1, dtype=torch.int64, device=dev)
    st = stream if stream is not None else _current_stream_handle()
    total = _u64(0)

    def call(out, cap):
        _check(L.ss_find_all_batched(haystacks.data_ptr(), hb, he, needles.data_ptr(), nb, ne, count, st,
                                     counts.data_ptr() if count else None, rows.data_ptr(), out.data_ptr() if cap else None, int(cap),
                                     ctypes.byref(total)), L)
    if capacity is None:
        call(None, 0)
        capacity = total.value
    out = torch.empty(max(int(capacity), 1), dtype=torch.int64, device=dev)
    call(out, capacity)
    return counts, rows, out[:min(int(capacity), total.value)]


def search_file(searcher, path):
    """examples/grep.rs:42-56: map the file, one search_in (row f2)."""
    found = ctypes.c_int(0)
    _check(searcher._L.ss_search_file(searcher._h, os.fsencode(path), ctypes.byref(found)), searcher._L)
    return bool(found.value)


def byte_histogram(haystack, sample_bytes=0, stream=None):
    """256 byte-value counts of a device haystack (row f3)."""
    hist = np.zeros(256, dtype=np.uint64)
    st = stream if stream is not None else _current_stream_handle()
    _check(lib().ss_byte_histogram_device(haystack.data_ptr(), haystack.numel(), sample_bytes, st, hist.ctypes.data))
    return hist


def choose_position(needle, hist=None):
    """Index of the rarest needle byte under `hist` (ties: later byte); no histogram -> n-1 (row f3)."""
    nb = bytes(needle)
    pos = _sz(0)
    h = None if hist is None else np.ascontiguousarray(hist, dtype=np.uint64)
    _check(lib().ss_choose_position(nb, len(nb), None if h is None else h.ctypes.data, ctypes.byref(pos)))
    return pos.value


def choose_filter_triple(needle, hist=None):
    """(first, second, third) that `DynamicHipSearcher.new(needle)` lets the device filter test; with `hist` (256
    byte counts of the haystack, `byte_histogram`) the corpus-aware choice to apply with `set_filter`."""
    nb = bytes(needle)
    a, b, c = _sz(0), _sz(0), _sz(0)
    h = None if hist is None else np.ascontiguousarray(hist, dtype=np.uint64)
    _check(lib().ss_choose_filter_triple(nb, len(nb), None if h is None else h.ctypes.data, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)))
    return a.value, b.value, c.value


def choose_filter_pair(needle):
    """(first, second): the first two of `choose_filter_triple(needle)`."""
    return choose_filter_triple(needle)[:2]


def choose_filter_for_position(needle, position):
    """(first, second, third) that `DynamicHipSearcher.with_position(needle, position)` lets the device filter test:
    `second == position`; `first == 0` (the reference's pair) when `position < 16`, else a byte at most 15 in front of it.
    Hooks builds (a pure host function; a constructed searcher's `filter3` says the same in every build)."""
    nb = bytes(needle)
    a, b, c = _sz(0), _sz(0), _sz(0)
    L = _feature_lib(lib(), "hooks")
    _check(L.ss_choose_filter_for_position(nb, len(nb), position, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)), L)
    return a.value, b.value, c.value


def fill_random_device(tensor, seed, global_offset=0, stream=None):
    st = stream if stream is not None else _current_stream_handle()
    _check_tools(tools_lib().ss_fill_random_device(tensor.data_ptr(), global_offset, tensor.numel(), seed, st))
    return tensor


def fill_random_host(length, seed, global_offset=0):
    out = np.empty(length, dtype=np.uint8)
    _check_tools(tools_lib().ss_fill_random_host(out.ctypes.data, global_offset, length, seed))
    return out


def read_ceiling_gbps(tensor, reps=10, stream=None):
    ms = ctypes.c_float(0)
    st = stream if stream is not None else _current_stream_handle()
    _check_tools(tools_lib().ss_read_ceiling(tensor.data_ptr(), tensor.numel(), st, reps, ctypes.byref(ms)))
    return tensor.numel() / (ms.value * 1e-3) / 1e9


def device_info():
    name = ctypes.create_string_buffer(256)
    cus, mem = ctypes.c_int(0), _sz(0)
    _check(lib().ss_device_info(name, 256, ctypes.byref(cus), ctypes.byref(mem)))
    return {"name": name.value.decode(), "compute_units": cus.value, "total_mem": mem.value}


def selftest_dpp():
    """320 uint32 of the cross-lane self-test (ss_selftest_dpp; tests/test_gpu_parity.py::test_cross_lane_primitives)."""
    out = np.zeros(320, dtype=np.uint32)
    _check_tools(tools_lib().ss_selftest_dpp(out.ctypes.data))
    return out
