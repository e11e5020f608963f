"""sliceslice-rs_amd - MI355X-native drop-in for the substring-search hot path of
cloudflare/sliceslice-rs (`DynamicAvx2Searcher::{new, with_position, search_in}`).

The product is the C-ABI shared library built from ``csrc/`` (declared in
``include/sliceslice_hip.h``); this package is the thin Python host-side mirror of
the reference interface used by the tests and by ``bench.py``.  The directory
name contains a hyphen, so import it through the repo-root shim::

    import sliceslice_rs_amd as ss
    s = ss.DynamicHipSearcher.new(b"ipsum")
    s.search_in(device_tensor_or_bytes)
"""
from ._build import build, library_path                      # noqa: F401
from .searcher import (                                      # noqa: F401
    SS_OK, SS_ERR_POSITION, SS_ERR_ARGUMENT, SS_ERR_NO_DEVICE, SS_ERR_HIP, SS_ERR_RCCL, SS_ERR_NOMEM, SS_ERR_PEER,
    DynamicHipSearcher, HipSearcher, MemchrHipSearcher, PositionError, SlicesliceError, ShardedSearcher, NodeSearcher, shard_range,
    SearchService, BatchPlan, tuning_build, service_build, matches_build, matches_batched_build, lines_build, nocase_build, bounded_build, inverted_build, context_build, lines_around, CONTEXT_PART_BYTES, SS_CONTEXT_INVERT, anyof_build, count_lines_anyof, find_lines_anyof, find_lines_anyof_into, union_numbers, union_numbers_into, ANYOF_MAX_NEEDLES, ANYOF_SEGMENT_LINES, needleset_build, setmatches_build, disjoint_build, select_disjoint, select_disjoint_into, DISJOINT_BLOCK, leftmost_build, select_leftmost, select_leftmost_into, LEFTMOST_BLOCK, masked_build, MaskedPattern, parse_hex, masked_choose_filter, MASKED_MAX_LEN, classes_build, ClassPattern, parse_classes, classes_cover, CLASSES_MAX_LEN, CLASSES_MAX_INEXACT, CLASSES_MAX_DISTINCT, runs_build, RunPattern, parse_runs, RUNS_MAX_LEN, RUNS_MAX_RANGES, SS_RUNS_BITMAP, rewrite_build, SS_REWRITE_MAX_TEXT, fields_build, FieldSelector, parse_fields, SS_FIELDS_EACH, SS_FIELDS_MERGE, SS_FIELDS_KEEP_SHORT, FIELDS_CARRY_CHUNK, groups_build, group_ranges, group_ranges_into, group_lines, group_lines_into, groups_scratch_bytes, SS_GROUPS_NOCASE, SS_GROUPS_WEAK_HASH, GROUPS_MAX_RANGES, GROUPS_BLOCK, GROUPS_LANE_MAX, GROUPS_LDS_BYTES, output_build, format_lines, format_lines_into, gather_ranges, grep_anyof, OUTPUT_BLOCK, OUTPUT_CHUNK, SS_OUTPUT_NUMBER, SS_OUTPUT_SEPARATOR, NeedleSet, SS_SET_NOCASE, fold_ascii, is_word_byte, set_autotune, rccl_info, TuningState, tools_lib, selftest_dpp,
    search_batched, find_batched, count_batched, find_all_batched, batch_classes, search_file, byte_histogram, choose_position, choose_filter_pair, choose_filter_triple, choose_filter_for_position, fill_random_device, fill_random_host, read_ceiling_gbps, device_info, lib,
)
