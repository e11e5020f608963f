// src/hip_nocase.rs - every occurrence of a needle, and the lines that contain it, ignoring ASCII case
// (include/sliceslice_hip_nocase.h): an OPT-IN component gated by a feature of its own
// (`#[cfg(feature = "hip-nocase")] pub mod hip_nocase;`).  A crate built with that feature links libsliceslice_hip_nocase.so - the
// lines library's objects plus the case-folding scans - INSTEAD of libsliceslice_hip.so (and may enable `hip-matches` and
// `hip-lines` next to it: the library holds those entry points too).
//
// SOURCE ONLY, like src/hip.rs: never compiled here (no rustc); the `extern "C"` block is checked mechanically against
// include/sliceslice_hip_nocase.h by tests/test_nocase_cpu.py.
#![allow(non_camel_case_types, dead_code)]
use crate::hip::{check, ss_searcher, DeviceSlice};
use crate::hip_lines::LineRecords;
use std::os::raw::{c_int, c_void};

extern "C" {
    pub fn ss_searcher_new_nocase(needle: *const u8, n: usize, out: *mut *mut ss_searcher) -> c_int;
    pub fn ss_count_nocase_device(s: *const ss_searcher, d_haystack: *const c_void, len: usize, hip_stream: *mut c_void,
                                  count: *mut u64) -> c_int;
    pub fn ss_count_nocase_device_async(s: *const ss_searcher, d_haystack: *const c_void, len: usize, hip_stream: *mut c_void,
                                        d_count: *mut u64) -> c_int;
    pub fn ss_find_all_nocase_device(s: *const ss_searcher, d_haystack: *const c_void, len: usize, hip_stream: *mut c_void,
                                     d_offsets: *mut u64, capacity: u64, count: *mut u64) -> c_int;
    pub fn ss_count_lines_nocase_device(s: *const ss_searcher, d_haystack: *const c_void, len: usize, delimiter: c_int,
                                        hip_stream: *mut c_void, lines: *mut u64) -> c_int;
    pub fn ss_count_lines_nocase_device_async(s: *const ss_searcher, d_haystack: *const c_void, len: usize, delimiter: c_int,
                                              hip_stream: *mut c_void, d_lines: *mut u64) -> c_int;
    pub fn ss_find_lines_nocase_device(s: *const ss_searcher, d_haystack: *const c_void, len: usize, delimiter: c_int,
                                       hip_stream: *mut c_void, d_begin: *mut u64, d_end: *mut u64, d_number: *mut u64, capacity: u64,
                                       lines: *mut u64) -> c_int;
}

/// A searcher for `needle.to_ascii_lowercase()`: what the calls below take.  It is an ordinary searcher of the nocase library;
/// the case-sensitive calls work on it with the folded needle.
pub struct NocaseSearcher {
    handle: *mut ss_searcher,
}

impl NocaseSearcher {
    pub fn new(needle: &[u8]) -> Self {
        let mut handle = std::ptr::null_mut();
        check(unsafe { ss_searcher_new_nocase(needle.as_ptr(), needle.len(), &mut handle) });
        NocaseSearcher { handle }
    }
    /// The number of (overlapping) occurrences, `eq_ignore_ascii_case` byte by byte.
    pub fn count_in(&self, haystack: DeviceSlice, stream: *mut c_void) -> u64 {
        let mut count = 0u64;
        check(unsafe { ss_count_nocase_device(self.handle, haystack.ptr, haystack.len, stream, &mut count) });
        count
    }
    /// The total, and the leftmost `min(total, capacity)` offsets in ascending order.
    pub fn find_all_in(&self, haystack: DeviceSlice, stream: *mut c_void, d_offsets: *mut u64, capacity: u64) -> u64 {
        let mut count = 0u64;
        check(unsafe { ss_find_all_nocase_device(self.handle, haystack.ptr, haystack.len, stream, d_offsets, capacity, &mut count) });
        count
    }
    /// The number of lines (cut at `delimiter`, which is never folded) that hold an occurrence.
    pub fn count_lines_in(&self, haystack: DeviceSlice, delimiter: u8, stream: *mut c_void) -> u64 {
        let mut lines = 0u64;
        check(unsafe { ss_count_lines_nocase_device(self.handle, haystack.ptr, haystack.len, delimiter as c_int, stream, &mut lines) });
        lines
    }
    pub fn find_lines_in(&self, haystack: DeviceSlice, delimiter: u8, stream: *mut c_void, out: &LineRecords) -> u64 {
        let mut lines = 0u64;
        check(unsafe {
            ss_find_lines_nocase_device(self.handle, haystack.ptr, haystack.len, delimiter as c_int, stream, out.d_begin, out.d_end,
                                        out.d_number, out.capacity, &mut lines)
        });
        lines
    }
}

impl Drop for NocaseSearcher {
    fn drop(&mut self) {
        unsafe { crate::hip::ss_searcher_free(self.handle) }
    }
}
