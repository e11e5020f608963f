// src/hip_runs.rs - the maximal runs of one byte class (`\w+`, `[0-9]{3,}`, `[A-Z]{2,5}`), counted and listed in ONE pass over the
// haystack (include/sliceslice_hip_runs.h has the rule and the language: a run is a maximal interval whose bytes are all in the set,
// selected when its length lies in [min_len, max_len]): an OPT-IN component gated by a feature of its own
// (`#[cfg(feature = "hip-runs")] pub mod hip_runs;`).  A crate built with that feature links libsliceslice_hip_runs.so - the
// classes library's objects plus the run scan - INSTEAD of libsliceslice_hip.so.
//
// SOURCE ONLY, like src/hip.rs: never compiled here (no rustc); the `extern "C"` block is checked mechanically against
// include/sliceslice_hip_runs.h by tests/test_runs_cpu.py.
#![allow(non_camel_case_types, dead_code)]
use crate::hip::{check, DeviceSlice};
use std::os::raw::{c_char, c_int, c_uint, c_void};

/// The largest min_len / max_len.
pub const SS_RUNS_MAX_LEN: u64 = 4096;
/// Maximal ranges of a set on the range path.
pub const SS_RUNS_MAX_RANGES: usize = 4;
/// ss_runs_new flag: force the bitmap path.
pub const SS_RUNS_BITMAP: c_uint = 1;

#[repr(C)]
pub struct ss_runs {
    _private: [u8; 0],
}

#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct ss_runs_stats {
    pub min_len: u64,
    pub max_len: u64,
    pub members: u64,
    pub ranges: u64,
    pub path: u64,
    pub accepts_delimiter: u64,
}

extern "C" {
    pub fn ss_runs_new(set: *const u64, min_len: u64, max_len: u64, flags: c_uint, runs: *mut *mut ss_runs) -> c_int;
    pub fn ss_runs_free(runs: *mut ss_runs);
    pub fn ss_runs_info(runs: *const ss_runs, delimiter: c_int, stats: *mut ss_runs_stats) -> c_int;
    pub fn ss_runs_parse(text: *const c_char, ignore_case: c_int, set: *mut u64, min_len: *mut u64, max_len: *mut u64) -> c_int;
    pub fn ss_count_runs_device(runs: *const ss_runs, d_haystack: *const c_void, len: usize, hip_stream: *mut c_void,
                                count: *mut u64) -> c_int;
    pub fn ss_count_runs_device_async(runs: *const ss_runs, d_haystack: *const c_void, len: usize, hip_stream: *mut c_void,
                                      d_count: *mut u64) -> c_int;
    pub fn ss_find_all_runs_device(runs: *const ss_runs, d_haystack: *const c_void, len: usize, hip_stream: *mut c_void,
                                   d_begin: *mut u64, d_end: *mut u64, capacity: u64, total: *mut u64) -> c_int;
    pub fn ss_count_lines_runs_device(runs: *const ss_runs, d_haystack: *const c_void, len: usize, delimiter: c_int,
                                      hip_stream: *mut c_void, lines: *mut u64) -> c_int;
    pub fn ss_find_lines_runs_device(runs: *const ss_runs, d_haystack: *const c_void, len: usize, delimiter: c_int,
                                     hip_stream: *mut c_void, d_begin: *mut u64, d_end: *mut u64, d_number: *mut u64, capacity: u64,
                                     lines: *mut u64) -> c_int;
}

/// A run pattern on the current device.
pub struct RunPattern {
    handle: *mut ss_runs,
}

impl RunPattern {
    /// `text`: one item of the classes language and one of `+ {k} {k,} {k,m}`, NUL-terminated by the caller's CString.
    pub fn new(text: &std::ffi::CStr, ignore_case: bool) -> Self {
        let (mut set, mut min_len, mut max_len) = ([0u64; 4], 0u64, 0u64);
        check(unsafe { ss_runs_parse(text.as_ptr(), ignore_case as c_int, set.as_mut_ptr(), &mut min_len, &mut max_len) });
        Self::from_set(&set, min_len, max_len, 0)
    }

    /// Four words: byte b is bit b & 63 of word b >> 6.  `max_len` 0: no maximum.
    pub fn from_set(set: &[u64; 4], min_len: u64, max_len: u64, flags: c_uint) -> Self {
        let mut handle = std::ptr::null_mut();
        check(unsafe { ss_runs_new(set.as_ptr(), min_len, max_len, flags, &mut handle) });
        RunPattern { handle }
    }

    /// The selected runs.
    pub fn count(&self, haystack: DeviceSlice, stream: *mut c_void) -> u64 {
        let mut count = 0u64;
        check(unsafe { ss_count_runs_device(self.handle, haystack.ptr, haystack.len, stream, &mut count) });
        count
    }

    /// The total; the leftmost `capacity` runs go to `d_begin` / `d_end` (either may be null).
    pub fn find_all(&self, haystack: DeviceSlice, stream: *mut c_void, d_begin: *mut u64, d_end: *mut u64, capacity: u64) -> u64 {
        let mut total = 0u64;
        check(unsafe { ss_find_all_runs_device(self.handle, haystack.ptr, haystack.len, stream, d_begin, d_end, capacity, &mut total) });
        total
    }

    /// The lines that hold a selected run; the delimiter is never a member.
    pub fn count_lines(&self, haystack: DeviceSlice, delimiter: u8, stream: *mut c_void) -> u64 {
        let mut lines = 0u64;
        check(unsafe { ss_count_lines_runs_device(self.handle, haystack.ptr, haystack.len, delimiter as c_int, stream, &mut lines) });
        lines
    }
}

impl Drop for RunPattern {
    fn drop(&mut self) {
        unsafe { ss_runs_free(self.handle) }
    }
}
