// src/hip_anyof.rs - the lines that match any of several needles, and the ordered union of ascending lists of line numbers
// (include/sliceslice_hip_anyof.h, grep -e A -e B / grep -f FILE): an OPT-IN component gated by a feature of its own
// (`#[cfg(feature = "hip-anyof")] pub mod hip_anyof;`).  A crate built with that feature links libsliceslice_hip_anyof.so - the
// context library's objects plus the union kernels - INSTEAD of libsliceslice_hip.so (and may enable `hip-matches`, `hip-lines`,
// `hip-nocase`, `hip-bounded`, `hip-inverted` and `hip-context` next to it: the library holds those entry points too).
//
// SOURCE ONLY, like src/hip.rs: never compiled here (no rustc); the `extern "C"` block is checked mechanically against
// include/sliceslice_hip_anyof.h by tests/test_anyof_cpu.py.
#![allow(non_camel_case_types, dead_code)]
use crate::hip::{check, ss_searcher, DeviceSlice};
use crate::hip_lines::LineRecords;
use std::os::raw::{c_int, c_uint, c_void};

/// Needles (or lists) per call.
pub const SS_ANYOF_MAX_NEEDLES: u32 = 65536;
/// Line numbers per workgroup of the union kernels.
pub const SS_ANYOF_SEGMENT_LINES: u64 = 65536;

extern "C" {
    pub fn ss_union_numbers_device(s: *const ss_searcher, d_numbers: *const u64, offsets: *const u64, lists: u32, limit: u64,
                                   complement: c_int, hip_stream: *mut c_void, d_out: *mut u64, capacity: u64, total: *mut u64) -> c_int;
    pub fn ss_count_lines_anyof_device(searchers: *const *const ss_searcher, needles: u32, d_haystack: *const c_void, len: usize,
                                       delimiter: c_int, how: c_uint, hip_stream: *mut c_void, lines: *mut u64) -> c_int;
    pub fn ss_find_lines_anyof_device(searchers: *const *const ss_searcher, needles: u32, d_haystack: *const c_void, len: usize,
                                      delimiter: c_int, how: c_uint, before: u64, after: u64, hip_stream: *mut c_void,
                                      d_begin: *mut u64, d_end: *mut u64, d_number: *mut u64, d_kind: *mut u8, capacity: u64,
                                      lines: *mut u64, selected: *mut u64) -> c_int;
}

/// The lines that match any of `searchers` under `how` (the bits of `hip_context`), counted.
pub fn count_lines_anyof(searchers: &[*const ss_searcher], haystack: DeviceSlice, delimiter: u8, how: c_uint, stream: *mut c_void) -> u64 {
    let mut lines = 0u64;
    check(unsafe {
        ss_count_lines_anyof_device(searchers.as_ptr(), searchers.len() as u32, haystack.ptr, haystack.len, delimiter as c_int, how, stream,
                                    &mut lines)
    });
    lines
}

/// (total, selected): the size of the output and the number of selected lines, as `hip_context::find_lines_with_context`.
pub fn find_lines_anyof(searchers: &[*const ss_searcher], haystack: DeviceSlice, delimiter: u8, how: c_uint, before: u64, after: u64,
                        stream: *mut c_void, out: &LineRecords, d_kind: *mut u8) -> (u64, u64) {
    let (mut lines, mut selected) = (0u64, 0u64);
    check(unsafe {
        ss_find_lines_anyof_device(searchers.as_ptr(), searchers.len() as u32, haystack.ptr, haystack.len, delimiter as c_int, how, before,
                                   after, stream, out.d_begin, out.d_end, out.d_number, d_kind, out.capacity, &mut lines, &mut selected)
    });
    (lines, selected)
}

/// The ascending union (or its complement in 1 ..= limit) of the strictly ascending lists `d_numbers[offsets[k] .. offsets[k + 1]]`.
pub fn union_numbers(s: *const ss_searcher, d_numbers: *const u64, offsets: &[u64], limit: u64, complement: bool, stream: *mut c_void,
                     d_out: *mut u64, capacity: u64) -> u64 {
    let mut total = 0u64;
    check(unsafe {
        ss_union_numbers_device(s, d_numbers, offsets.as_ptr(), (offsets.len() - 1) as u32, limit, complement as c_int, stream, d_out,
                                capacity, &mut total)
    });
    total
}
