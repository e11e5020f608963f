// src/hip_masked.rs - byte patterns with wildcards and per-byte masks, searched in ONE pass over the haystack
// (include/sliceslice_hip_masked.h has the rule: position p matches when (hay[p + i] & mask[i]) == value[i] for every i; what YARA
// and ClamAV hex strings, a `.` inside a literal and a needle in either case come down to): an OPT-IN component gated by a feature
// of its own (`#[cfg(feature = "hip-masked")] pub mod hip_masked;`).  A crate built with that feature links
// libsliceslice_hip_masked.so - the leftmost library's objects plus the masked scan - INSTEAD of libsliceslice_hip.so.
//
// SOURCE ONLY, like src/hip.rs: never compiled here (no rustc); the `extern "C"` block is checked mechanically against
// include/sliceslice_hip_masked.h by tests/test_masked_cpu.py.
#![allow(non_camel_case_types, dead_code)]
use crate::hip::{check, DeviceSlice};
use std::os::raw::{c_char, c_int, c_void};

/// Bytes of a pattern.
pub const SS_MASKED_MAX_LEN: usize = 4096;

#[repr(C)]
pub struct ss_masked {
    _private: [u8; 0],
}

#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct ss_masked_stats {
    pub n: u64,
    pub anchor: u64,
    pub distance: u64,
    pub full: u64,
    pub partial: u64,
    pub wild: u64,
    pub accepts_delimiter: u64,
    pub reserved: u64,
}

extern "C" {
    pub fn ss_masked_new(value: *const c_void, mask: *const c_void, n: usize, pattern: *mut *mut ss_masked) -> c_int;
    pub fn ss_masked_free(pattern: *mut ss_masked);
    pub fn ss_masked_info(pattern: *const ss_masked, delimiter: c_int, stats: *mut ss_masked_stats) -> c_int;
    pub fn ss_masked_parse_hex(text: *const c_char, value: *mut u8, mask: *mut u8, capacity: usize, n: *mut usize) -> c_int;
    pub fn ss_masked_choose_filter(value: *const c_void, mask: *const c_void, n: usize, hist: *const u64, anchor: *mut usize,
                                   distance: *mut usize) -> c_int;
    pub fn ss_count_masked_device(pattern: *const ss_masked, d_haystack: *const c_void, len: usize, hip_stream: *mut c_void,
                                  count: *mut u64) -> c_int;
    pub fn ss_count_masked_device_async(pattern: *const ss_masked, d_haystack: *const c_void, len: usize, hip_stream: *mut c_void,
                                        d_count: *mut u64) -> c_int;
    pub fn ss_find_all_masked_device(pattern: *const ss_masked, d_haystack: *const c_void, len: usize, hip_stream: *mut c_void,
                                     d_offsets: *mut u64, capacity: u64, total: *mut u64) -> c_int;
    pub fn ss_count_lines_masked_device(pattern: *const ss_masked, d_haystack: *const c_void, len: usize, delimiter: c_int,
                                        hip_stream: *mut c_void, lines: *mut u64) -> c_int;
    pub fn ss_find_lines_masked_device(pattern: *const ss_masked, d_haystack: *const c_void, len: usize, delimiter: c_int,
                                       hip_stream: *mut c_void, d_begin: *mut u64, d_end: *mut u64, d_number: *mut u64, capacity: u64,
                                       lines: *mut u64) -> c_int;
}

/// A compiled pattern on the current device; `mask` empty means all 0xFF.
pub struct MaskedPattern {
    handle: *mut ss_masked,
}

impl MaskedPattern {
    pub fn new(value: &[u8], mask: &[u8]) -> Self {
        assert!(mask.is_empty() || mask.len() == value.len());
        let mut handle = std::ptr::null_mut();
        let m = if mask.is_empty() { std::ptr::null() } else { mask.as_ptr() as *const c_void };
        check(unsafe { ss_masked_new(value.as_ptr() as *const c_void, m, value.len(), &mut handle) });
        MaskedPattern { handle }
    }

    /// The occurrences, overlapping ones included.
    pub fn count(&self, haystack: DeviceSlice, stream: *mut c_void) -> u64 {
        let mut count = 0u64;
        check(unsafe { ss_count_masked_device(self.handle, haystack.ptr, haystack.len, stream, &mut count) });
        count
    }

    /// The total; the leftmost `capacity` offsets go to `d_offsets`.
    pub fn find_all(&self, haystack: DeviceSlice, stream: *mut c_void, d_offsets: *mut u64, capacity: u64) -> u64 {
        let mut total = 0u64;
        check(unsafe { ss_find_all_masked_device(self.handle, haystack.ptr, haystack.len, stream, d_offsets, capacity, &mut total) });
        total
    }

    /// The lines that hold an occurrence wholly inside them.
    pub fn count_lines(&self, haystack: DeviceSlice, delimiter: u8, stream: *mut c_void) -> u64 {
        let mut lines = 0u64;
        check(unsafe { ss_count_lines_masked_device(self.handle, haystack.ptr, haystack.len, delimiter as c_int, stream, &mut lines) });
        lines
    }
}

impl Drop for MaskedPattern {
    fn drop(&mut self) {
        unsafe { ss_masked_free(self.handle) }
    }
}
