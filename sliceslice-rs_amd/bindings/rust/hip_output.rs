// src/hip_output.rs - grep's OUTPUT written on the device: the text of a list of records gathered into one buffer, with line numbers,
// `:` / `-`, terminators and `--` separators (include/sliceslice_hip_output.h; what `grep -n -A / -B / -C -F needle file` writes to
// stdout, and the gather behind `grep -o` and `sed -n 'Np'`): an OPT-IN component gated by a feature of its own
// (`#[cfg(feature = "hip-output")] pub mod hip_output;`).  A crate built with that feature links libsliceslice_hip_output.so - the
// disjoint library's objects plus the output kernels - INSTEAD of libsliceslice_hip.so (and enables `hip-bounded` and `hip-context`
// next to it: the `how` bits are defined there, and the library holds those entry points too).
//
// SOURCE ONLY, like src/hip.rs: never compiled here (no rustc); the `extern "C"` block is checked mechanically against
// include/sliceslice_hip_output.h by tests/test_output_cpu.py.
#![allow(non_camel_case_types, dead_code)]
use crate::hip::{check, ss_searcher, DeviceSlice};
use std::os::raw::{c_int, c_uint, c_void};

/// flags: `number:` / `number-` in front of every record's text.
pub const SS_OUTPUT_NUMBER: c_uint = 1;
/// flags: `--` wherever two consecutive numbers differ by more than 1.
pub const SS_OUTPUT_SEPARATOR: c_uint = 2;
/// Records per workgroup of the size passes.
pub const SS_OUTPUT_BLOCK: u64 = 4096;
/// Output bytes per workgroup of the copy pass.
pub const SS_OUTPUT_CHUNK: u64 = 16384;

extern "C" {
    pub fn ss_format_lines_device(s: *const ss_searcher, d_haystack: *const c_void, len: usize, d_begin: *const u64, d_end: *const u64,
                                  d_number: *const u64, d_kind: *const u8, count: u64, terminator: c_int, flags: c_uint,
                                  hip_stream: *mut c_void, d_out: *mut c_void, out_capacity: u64, d_starts: *mut u64,
                                  out_len: *mut u64) -> c_int;
    pub fn ss_gather_ranges_device(s: *const ss_searcher, d_haystack: *const c_void, len: usize, d_begin: *const u64, d_end: *const u64,
                                   count: u64, terminator: c_int, hip_stream: *mut c_void, d_out: *mut c_void, out_capacity: u64,
                                   d_starts: *mut u64, out_len: *mut u64) -> c_int;
    pub fn ss_grep_lines_device(s: *const ss_searcher, d_haystack: *const c_void, len: usize, delimiter: c_int, how: c_uint, before: u64,
                                after: u64, flags: c_uint, hip_stream: *mut c_void, d_out: *mut c_void, out_capacity: u64,
                                out_len: *mut u64, lines: *mut u64, selected: *mut u64) -> c_int;
}

/// The records of a line call in device memory: `count` entries each; `number` may be null without flags, `kind` may be null (every
/// record prints `:`).
#[derive(Clone, Copy)]
pub struct DeviceRecords {
    pub begin: *const u64,
    pub end: *const u64,
    pub number: *const u64,
    pub kind: *const u8,
    pub count: u64,
}

fn terminator_of(terminator: Option<u8>) -> c_int {
    match terminator {
        Some(byte) => byte as c_int,
        None => -1,
    }
}

/// The length of the records' text with `flags`; the bytes are written to `d_out` when `out_capacity` holds them, nothing is written
/// otherwise.  `d_starts` (may be null) receives the `count + 1` output offsets at which the records begin.  `s` names the device only.
pub fn format_lines(s: *const ss_searcher, haystack: DeviceSlice, records: DeviceRecords, terminator: Option<u8>, flags: c_uint,
                    stream: *mut c_void, d_out: *mut c_void, out_capacity: u64, d_starts: *mut u64) -> u64 {
    let mut out_len = 0u64;
    check(unsafe {
        ss_format_lines_device(s, haystack.ptr, haystack.len, records.begin, records.end, records.number, records.kind, records.count,
                               terminator_of(terminator), flags, stream, d_out, out_capacity, d_starts, &mut out_len)
    });
    out_len
}

/// The same without numbers: the bytes `[begin[i], end[i])` of the haystack, clamped to it, each followed by the terminator.
pub fn gather_ranges(s: *const ss_searcher, haystack: DeviceSlice, d_begin: *const u64, d_end: *const u64, count: u64,
                     terminator: Option<u8>, stream: *mut c_void, d_out: *mut c_void, out_capacity: u64, d_starts: *mut u64) -> u64 {
    let mut out_len = 0u64;
    check(unsafe {
        ss_gather_ranges_device(s, haystack.ptr, haystack.len, d_begin, d_end, count, terminator_of(terminator), stream, d_out, out_capacity,
                                d_starts, &mut out_len)
    });
    out_len
}

/// (out_len, lines, selected) of `grep -F needle` with `before` / `after` context lines: what it writes to stdout goes to `d_out`
/// when `out_capacity` holds it.  `how` takes the bits of `hip_context::find_lines_context`.
pub fn grep_lines(s: *const ss_searcher, haystack: DeviceSlice, delimiter: u8, how: c_uint, before: u64, after: u64, flags: c_uint,
                  stream: *mut c_void, d_out: *mut c_void, out_capacity: u64) -> (u64, u64, u64) {
    let (mut out_len, mut lines, mut selected) = (0u64, 0u64, 0u64);
    check(unsafe {
        ss_grep_lines_device(s, haystack.ptr, haystack.len, delimiter as c_int, how, before, after, flags, stream, d_out, out_capacity,
                             &mut out_len, &mut lines, &mut selected)
    });
    (out_len, lines, selected)
}
