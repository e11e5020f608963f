// src/hip_inverted.rs - the lines that do NOT match: their number and their records (include/sliceslice_hip_inverted.h, grep -v
// with -c and -n): an OPT-IN component gated by a feature of its own (`#[cfg(feature = "hip-inverted")] pub mod hip_inverted;`).
// A crate built with that feature links libsliceslice_hip_inverted.so - the bounded library's objects plus the inverted kernels -
// INSTEAD of libsliceslice_hip.so (and may enable `hip-matches`, `hip-lines`, `hip-nocase` and `hip-bounded` next to it: the library
// holds those entry points too).  There is no inverted occurrence form: occurrences have no complement.
//
// SOURCE ONLY, like src/hip.rs: never compiled here (no rustc); the `extern "C"` block is checked mechanically against
// include/sliceslice_hip_inverted.h by tests/test_inverted_cpu.py.
#![allow(non_camel_case_types, dead_code)]
use crate::hip::{check, ss_searcher, DeviceSlice};
use crate::hip_bounded::{SS_BOUND_LINE, SS_BOUND_NOCASE, SS_BOUND_WORD};
use crate::hip_lines::LineRecords;
use std::os::raw::{c_int, c_uint, c_void};

extern "C" {
    pub fn ss_count_lines_inverted_device(s: *const ss_searcher, d_haystack: *const c_void, len: usize, delimiter: c_int, how: c_uint,
                                          hip_stream: *mut c_void, lines: *mut u64) -> c_int;
    pub fn ss_count_lines_inverted_device_async(s: *const ss_searcher, d_haystack: *const c_void, len: usize, delimiter: c_int,
                                                how: c_uint, hip_stream: *mut c_void, d_lines: *mut u64) -> c_int;
    pub fn ss_find_lines_inverted_device(s: *const ss_searcher, d_haystack: *const c_void, len: usize, delimiter: c_int, how: c_uint,
                                         hip_stream: *mut c_void, d_begin: *mut u64, d_end: *mut u64, d_number: *mut u64, capacity: u64,
                                         lines: *mut u64) -> c_int;
}

/// The non-inverted call whose complement is taken: plain, whole word or whole line, each with or without ASCII case folding
/// (`nocase` needs a needle without 'A'..'Z': `hip_nocase::NocaseSearcher` folds one).
#[derive(Clone, Copy, PartialEq)]
pub enum Match {
    Anywhere,
    WholeWord,
    WholeLine,
}

fn how(m: Match, nocase: bool) -> c_uint {
    (match m {
        Match::Anywhere => 0,
        Match::WholeWord => SS_BOUND_WORD,
        Match::WholeLine => SS_BOUND_LINE,
    }) | (if nocase { SS_BOUND_NOCASE } else { 0 })
}

/// The number of lines (cut at `delimiter`) that do NOT match: grep -v -c, with -w / -x / -i as `m` and `nocase` say.
pub fn count_lines_not_in(s: *const ss_searcher, haystack: DeviceSlice, delimiter: u8, m: Match, nocase: bool, stream: *mut c_void) -> u64 {
    let mut lines = 0u64;
    check(unsafe { ss_count_lines_inverted_device(s, haystack.ptr, haystack.len, delimiter as c_int, how(m, nocase), stream, &mut lines) });
    lines
}

/// The total, and the records of the leftmost `min(total, out.capacity)` lines that do not match, in ascending order.
pub fn find_lines_not_in(s: *const ss_searcher, haystack: DeviceSlice, delimiter: u8, m: Match, nocase: bool, stream: *mut c_void,
                         out: &LineRecords) -> u64 {
    let mut lines = 0u64;
    check(unsafe {
        ss_find_lines_inverted_device(s, haystack.ptr, haystack.len, delimiter as c_int, how(m, nocase), stream, out.d_begin, out.d_end,
                                      out.d_number, out.capacity, &mut lines)
    });
    lines
}
