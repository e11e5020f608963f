// src/hip_context.rs - matching lines with their context lines, and the records of any set of line numbers
// (include/sliceslice_hip_context.h, grep -A / -B / -C with -n): an OPT-IN component gated by a feature of its own
// (`#[cfg(feature = "hip-context")] pub mod hip_context;`).  A crate built with that feature links libsliceslice_hip_context.so - the
// inverted library's objects plus the context kernels - INSTEAD of libsliceslice_hip.so (and may enable `hip-matches`, `hip-lines`,
// `hip-nocase`, `hip-bounded` and `hip-inverted` next to it: the library holds those entry points too).
//
// SOURCE ONLY, like src/hip.rs: never compiled here (no rustc); the `extern "C"` block is checked mechanically against
// include/sliceslice_hip_context.h by tests/test_context_cpu.py.
#![allow(non_camel_case_types, dead_code)]
use crate::hip::{check, ss_searcher, DeviceSlice};
use crate::hip_bounded::{SS_BOUND_LINE, SS_BOUND_NOCASE, SS_BOUND_WORD};
use crate::hip_lines::LineRecords;
use std::os::raw::{c_int, c_uint, c_void};

/// With the SS_BOUND_* bits in `how`: the model is the inverted call.
pub const SS_CONTEXT_INVERT: c_uint = 8;
/// Bytes of the view per workgroup of the delimiter census and the select pass.
pub const SS_CONTEXT_PART_BYTES: usize = 65536;

extern "C" {
    pub fn ss_lines_around_device(s: *const ss_searcher, d_haystack: *const c_void, len: usize, delimiter: c_int, d_numbers: *const u64,
                                  count: u64, before: u64, after: u64, hip_stream: *mut c_void, d_begin: *mut u64, d_end: *mut u64,
                                  d_number: *mut u64, d_kind: *mut u8, capacity: u64, lines: *mut u64) -> c_int;
    pub fn ss_find_lines_context_device(s: *const ss_searcher, d_haystack: *const c_void, len: usize, delimiter: c_int, how: c_uint,
                                        before: u64, after: u64, hip_stream: *mut c_void, d_begin: *mut u64, d_end: *mut u64,
                                        d_number: *mut u64, d_kind: *mut u8, capacity: u64, lines: *mut u64, selected: *mut u64) -> c_int;
}

/// The model call whose lines are selected: plain, whole word or whole line, each with or without ASCII case folding and each
/// inverted or not (`nocase` needs a needle without 'A'..'Z': `hip_nocase::NocaseSearcher` folds one).
#[derive(Clone, Copy, PartialEq)]
pub enum Match {
    Anywhere,
    WholeWord,
    WholeLine,
}

fn how(m: Match, nocase: bool, invert: bool) -> c_uint {
    (match m {
        Match::Anywhere => 0,
        Match::WholeWord => SS_BOUND_WORD,
        Match::WholeLine => SS_BOUND_LINE,
    }) | (if nocase { SS_BOUND_NOCASE } else { 0 }) | (if invert { SS_CONTEXT_INVERT } else { 0 })
}

/// (total, selected): the size of the output and the number of selected lines.  The records of the leftmost
/// `min(total, out.capacity)` output lines go to `out`, their kinds (1: selected, 0: context) to `d_kind` (may be null).
pub fn find_lines_with_context(s: *const ss_searcher, haystack: DeviceSlice, delimiter: u8, m: Match, nocase: bool, invert: bool,
                               before: u64, after: u64, stream: *mut c_void, out: &LineRecords, d_kind: *mut u8) -> (u64, u64) {
    let (mut lines, mut selected) = (0u64, 0u64);
    check(unsafe {
        ss_find_lines_context_device(s, haystack.ptr, haystack.len, delimiter as c_int, how(m, nocase, invert), before, after, stream,
                                     out.d_begin, out.d_end, out.d_number, d_kind, out.capacity, &mut lines, &mut selected)
    });
    (lines, selected)
}

/// The same for `count` strictly ascending 1-based line numbers in device memory; `s` names the device only.
pub fn lines_around(s: *const ss_searcher, haystack: DeviceSlice, delimiter: u8, d_numbers: *const u64, count: u64, before: u64,
                    after: u64, stream: *mut c_void, out: &LineRecords, d_kind: *mut u8) -> u64 {
    let mut lines = 0u64;
    check(unsafe {
        ss_lines_around_device(s, haystack.ptr, haystack.len, delimiter as c_int, d_numbers, count, before, after, stream, out.d_begin,
                               out.d_end, out.d_number, d_kind, out.capacity, &mut lines)
    });
    lines
}
