// src/hip_bounded.rs - every occurrence of a needle, and the lines that contain it, kept only where the needle stands as a whole
// word or is the whole line (include/sliceslice_hip_bounded.h): an OPT-IN component gated by a feature of its own
// (`#[cfg(feature = "hip-bounded")] pub mod hip_bounded;`).  A crate built with that feature links libsliceslice_hip_bounded.so -
// the nocase library's objects plus the bounded scans - INSTEAD of libsliceslice_hip.so (and may enable `hip-matches`, `hip-lines`
// and `hip-nocase` next to it: the library holds those entry points too).
//
// SOURCE ONLY, like src/hip.rs: never compiled here (no rustc); the `extern "C"` block is checked mechanically against
// include/sliceslice_hip_bounded.h by tests/test_bounded_cpu.py.
#![allow(non_camel_case_types, dead_code)]
use crate::hip::{check, ss_searcher, DeviceSlice};
use crate::hip_lines::LineRecords;
use std::os::raw::{c_int, c_uint, c_void};

pub const SS_BOUND_WORD: c_uint = 1;
pub const SS_BOUND_LINE: c_uint = 2;
pub const SS_BOUND_NOCASE: c_uint = 4;

extern "C" {
    pub fn ss_count_bounded_device(s: *const ss_searcher, d_haystack: *const c_void, len: usize, how: c_uint, hip_stream: *mut c_void,
                                   count: *mut u64) -> c_int;
    pub fn ss_count_bounded_device_async(s: *const ss_searcher, d_haystack: *const c_void, len: usize, how: c_uint,
                                         hip_stream: *mut c_void, d_count: *mut u64) -> c_int;
    pub fn ss_find_all_bounded_device(s: *const ss_searcher, d_haystack: *const c_void, len: usize, how: c_uint, hip_stream: *mut c_void,
                                      d_offsets: *mut u64, capacity: u64, count: *mut u64) -> c_int;
    pub fn ss_count_lines_bounded_device(s: *const ss_searcher, d_haystack: *const c_void, len: usize, delimiter: c_int, how: c_uint,
                                         hip_stream: *mut c_void, lines: *mut u64) -> c_int;
    pub fn ss_count_lines_bounded_device_async(s: *const ss_searcher, d_haystack: *const c_void, len: usize, delimiter: c_int,
                                               how: c_uint, hip_stream: *mut c_void, d_lines: *mut u64) -> c_int;
    pub fn ss_find_lines_bounded_device(s: *const ss_searcher, d_haystack: *const c_void, len: usize, delimiter: c_int, how: c_uint,
                                        hip_stream: *mut c_void, d_begin: *mut u64, d_end: *mut u64, d_number: *mut u64, capacity: u64,
                                        lines: *mut u64) -> c_int;
}

/// What the calls below keep: an occurrence that stands as a word, or one that is its whole line (line forms only); `nocase`
/// compares letters in either case and needs a needle without 'A'..'Z' (`hip_nocase::NocaseSearcher` folds one).
#[derive(Clone, Copy)]
pub struct Bound {
    pub whole_line: bool,
    pub nocase: bool,
}

impl Bound {
    fn how(self) -> c_uint {
        (if self.whole_line { SS_BOUND_LINE } else { SS_BOUND_WORD }) | (if self.nocase { SS_BOUND_NOCASE } else { 0 })
    }
}

/// The number of (overlapping) whole-word occurrences of the searcher's needle: both neighbour bytes absent or outside [0-9A-Za-z_].
pub fn count_words_in(s: *const ss_searcher, haystack: DeviceSlice, nocase: bool, stream: *mut c_void) -> u64 {
    let mut count = 0u64;
    let how = Bound { whole_line: false, nocase }.how();
    check(unsafe { ss_count_bounded_device(s, haystack.ptr, haystack.len, how, stream, &mut count) });
    count
}

/// The total, and the leftmost `min(total, capacity)` whole-word offsets in ascending order.
pub fn find_all_words_in(s: *const ss_searcher, haystack: DeviceSlice, nocase: bool, stream: *mut c_void, d_offsets: *mut u64,
                         capacity: u64) -> u64 {
    let mut count = 0u64;
    let how = Bound { whole_line: false, nocase }.how();
    check(unsafe { ss_find_all_bounded_device(s, haystack.ptr, haystack.len, how, stream, d_offsets, capacity, &mut count) });
    count
}

/// The number of lines (cut at `delimiter`) that hold a kept occurrence: grep -w -c, or grep -x -c with `bound.whole_line`.
pub fn count_lines_in(s: *const ss_searcher, haystack: DeviceSlice, delimiter: u8, bound: Bound, stream: *mut c_void) -> u64 {
    let mut lines = 0u64;
    check(unsafe { ss_count_lines_bounded_device(s, haystack.ptr, haystack.len, delimiter as c_int, bound.how(), stream, &mut lines) });
    lines
}

pub fn find_lines_in(s: *const ss_searcher, haystack: DeviceSlice, delimiter: u8, bound: Bound, stream: *mut c_void,
                     out: &LineRecords) -> u64 {
    let mut lines = 0u64;
    check(unsafe {
        ss_find_lines_bounded_device(s, haystack.ptr, haystack.len, delimiter as c_int, bound.how(), stream, out.d_begin, out.d_end,
                                     out.d_number, out.capacity, &mut lines)
    });
    lines
}
