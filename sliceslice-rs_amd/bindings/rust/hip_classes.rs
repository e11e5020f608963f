// src/hip_classes.rs - fixed-length patterns of byte classes (`[0-9]{3}`, `\d\d:\d\d`, `[0-9A-F]{4}H`), searched in ONE pass over
// the haystack (include/sliceslice_hip_classes.h has the rule and the pattern language: position p matches when hay[p + i] is in
// set i for every i, a set being 256 bits in four words): an OPT-IN component gated by a feature of its own
// (`#[cfg(feature = "hip-classes")] pub mod hip_classes;`).  A crate built with that feature links
// libsliceslice_hip_classes.so - the masked library's objects plus the class scan - INSTEAD of libsliceslice_hip.so.
//
// SOURCE ONLY, like src/hip.rs: never compiled here (no rustc); the `extern "C"` block is checked mechanically against
// include/sliceslice_hip_classes.h by tests/test_classes_cpu.py.
#![allow(non_camel_case_types, dead_code)]
use crate::hip::{check, DeviceSlice};
use std::os::raw::{c_char, c_int, c_void};

/// Positions of a pattern.
pub const SS_CLASSES_MAX_LEN: usize = 4096;
/// Positions whose set is not exactly what its cover accepts.
pub const SS_CLASSES_MAX_INEXACT: usize = 1024;
/// Distinct sets among them.
pub const SS_CLASSES_MAX_DISTINCT: usize = 64;

#[repr(C)]
pub struct ss_classes {
    _private: [u8; 0],
}

#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct ss_classes_stats {
    pub n: u64,
    pub anchor: u64,
    pub distance: u64,
    pub single: u64,
    pub masked: u64,
    pub inexact: u64,
    pub distinct: u64,
    pub accepts_delimiter: u64,
}

extern "C" {
    pub fn ss_classes_new(sets: *const u64, n: usize, pattern: *mut *mut ss_classes) -> c_int;
    pub fn ss_classes_free(pattern: *mut ss_classes);
    pub fn ss_classes_info(pattern: *const ss_classes, delimiter: c_int, stats: *mut ss_classes_stats) -> c_int;
    pub fn ss_classes_parse(text: *const c_char, ignore_case: c_int, sets: *mut u64, capacity: usize, n: *mut usize) -> c_int;
    pub fn ss_classes_cover(sets: *const u64, n: usize, value: *mut u8, mask: *mut u8) -> c_int;
    pub fn ss_count_classes_device(pattern: *const ss_classes, d_haystack: *const c_void, len: usize, hip_stream: *mut c_void,
                                   count: *mut u64) -> c_int;
    pub fn ss_count_classes_device_async(pattern: *const ss_classes, d_haystack: *const c_void, len: usize, hip_stream: *mut c_void,
                                         d_count: *mut u64) -> c_int;
    pub fn ss_find_all_classes_device(pattern: *const ss_classes, d_haystack: *const c_void, len: usize, hip_stream: *mut c_void,
                                      d_offsets: *mut u64, capacity: u64, total: *mut u64) -> c_int;
    pub fn ss_count_lines_classes_device(pattern: *const ss_classes, d_haystack: *const c_void, len: usize, delimiter: c_int,
                                         hip_stream: *mut c_void, lines: *mut u64) -> c_int;
    pub fn ss_find_lines_classes_device(pattern: *const ss_classes, d_haystack: *const c_void, len: usize, delimiter: c_int,
                                        hip_stream: *mut c_void, d_begin: *mut u64, d_end: *mut u64, d_number: *mut u64, capacity: u64,
                                        lines: *mut u64) -> c_int;
}

/// A compiled pattern on the current device.
pub struct ClassPattern {
    handle: *mut ss_classes,
}

impl ClassPattern {
    /// `text` in the pattern language of the header, NUL-terminated by the caller's CString.
    pub fn new(text: &std::ffi::CStr, ignore_case: bool) -> Self {
        let mut n = 0usize;
        check(unsafe { ss_classes_parse(text.as_ptr(), ignore_case as c_int, std::ptr::null_mut(), 0, &mut n) });
        let mut sets = vec![0u64; 4 * n.max(1)];
        check(unsafe { ss_classes_parse(text.as_ptr(), ignore_case as c_int, sets.as_mut_ptr(), n, &mut n) });
        Self::from_sets(&sets[..4 * n])
    }

    /// Four words per position: byte b is bit b & 63 of word b >> 6.
    pub fn from_sets(sets: &[u64]) -> Self {
        assert!(sets.len() % 4 == 0);
        let mut handle = std::ptr::null_mut();
        check(unsafe { ss_classes_new(sets.as_ptr(), sets.len() / 4, &mut handle) });
        ClassPattern { handle }
    }

    /// The occurrences, overlapping ones included.
    pub fn count(&self, haystack: DeviceSlice, stream: *mut c_void) -> u64 {
        let mut count = 0u64;
        check(unsafe { ss_count_classes_device(self.handle, haystack.ptr, haystack.len, stream, &mut count) });
        count
    }

    /// The total; the leftmost `capacity` offsets go to `d_offsets`.
    pub fn find_all(&self, haystack: DeviceSlice, stream: *mut c_void, d_offsets: *mut u64, capacity: u64) -> u64 {
        let mut total = 0u64;
        check(unsafe { ss_find_all_classes_device(self.handle, haystack.ptr, haystack.len, stream, d_offsets, capacity, &mut total) });
        total
    }

    /// The lines that hold an occurrence wholly inside them.
    pub fn count_lines(&self, haystack: DeviceSlice, delimiter: u8, stream: *mut c_void) -> u64 {
        let mut lines = 0u64;
        check(unsafe { ss_count_lines_classes_device(self.handle, haystack.ptr, haystack.len, delimiter as c_int, stream, &mut lines) });
        lines
    }
}

impl Drop for ClassPattern {
    fn drop(&mut self) {
        unsafe { ss_classes_free(self.handle) }
    }
}
