// src/hip_lines.rs - the lines that contain a needle (include/sliceslice_hip_lines.h): count and records, an OPT-IN component gated
// by a feature of its own (`#[cfg(feature = "hip-lines")] pub mod hip_lines;`).  A crate built with that feature links
// libsliceslice_hip_lines.so - the matches library's objects plus the matching-lines scan - INSTEAD of libsliceslice_hip.so (and
// may enable `hip-matches` next to it: the library holds those entry points too).
//
// SOURCE ONLY, like src/hip.rs: never compiled here (no rustc); the `extern "C"` block is checked mechanically against
// include/sliceslice_hip_lines.h by tests/test_lines_cpu.py.
#![allow(non_camel_case_types, dead_code)]
use crate::hip::{check, ss_searcher, DeviceSlice, DynamicHipSearcher};
use crate::Needle;
use std::os::raw::{c_int, c_void};

extern "C" {
    pub fn ss_count_lines_device(s: *const ss_searcher, d_haystack: *const c_void, len: usize, delimiter: c_int, hip_stream: *mut c_void,
                                 lines: *mut u64) -> c_int;
    pub fn ss_count_lines_device_async(s: *const ss_searcher, d_haystack: *const c_void, len: usize, delimiter: c_int, hip_stream: *mut c_void,
                                       d_lines: *mut u64) -> c_int;
    pub fn ss_find_lines_device(s: *const ss_searcher, d_haystack: *const c_void, len: usize, delimiter: c_int, hip_stream: *mut c_void,
                                d_begin: *mut u64, d_end: *mut u64, d_number: *mut u64, capacity: u64, lines: *mut u64) -> c_int;
}

/// Device buffers for the records of the matching lines; a null pointer means "that array is not wanted".
pub struct LineRecords {
    pub d_begin: *mut u64,
    pub d_end: *mut u64,
    pub d_number: *mut u64,
    pub capacity: u64,
}

/// The lines of a haystack cut at every `delimiter` byte that hold at least one occurrence of the needle: `grep -c` and `grep -n`.
/// A needle that holds the delimiter matches no line; the empty needle matches every line.  The searcher must come from the lines
/// library (a crate built with `hip-lines`).
pub trait MatchingLines {
    /// The number of matching lines of a device-resident haystack.
    fn count_lines_in(&self, haystack: DeviceSlice, delimiter: u8, stream: *mut c_void) -> u64;
    /// The total, and the leftmost `min(total, capacity)` records - first byte, closing delimiter (or len), 1-based line number -
    /// in ascending order; nothing at index `capacity` or beyond is written.
    fn find_lines_in(&self, haystack: DeviceSlice, delimiter: u8, stream: *mut c_void, out: &LineRecords) -> u64;
}

impl<N: Needle> MatchingLines for DynamicHipSearcher<N> {
    fn count_lines_in(&self, haystack: DeviceSlice, delimiter: u8, stream: *mut c_void) -> u64 {
        let mut lines = 0u64;
        check(unsafe { ss_count_lines_device(self.handle(), haystack.ptr, haystack.len, delimiter as c_int, stream, &mut lines) });
        lines
    }
    fn find_lines_in(&self, haystack: DeviceSlice, delimiter: u8, stream: *mut c_void, out: &LineRecords) -> u64 {
        let mut lines = 0u64;
        check(unsafe {
            ss_find_lines_device(self.handle(), haystack.ptr, haystack.len, delimiter as c_int, stream, out.d_begin, out.d_end, out.d_number,
                                 out.capacity, &mut lines)
        });
        lines
    }
}
