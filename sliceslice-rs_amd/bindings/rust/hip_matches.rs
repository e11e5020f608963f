// src/hip_matches.rs - every occurrence of a needle (include/sliceslice_hip_matches.h): count and find-all, an OPT-IN component
// gated by a feature of its own (`#[cfg(feature = "hip-matches")] pub mod hip_matches;`).  A crate built with that feature links
// libsliceslice_hip_matches.so - the drop-in library's objects plus the all-matches scan - INSTEAD of libsliceslice_hip.so.
//
// SOURCE ONLY, like src/hip.rs: never compiled here (no rustc); the `extern "C"` block is checked mechanically against
// include/sliceslice_hip_matches.h by tests/test_matches_cpu.py.
#![allow(non_camel_case_types, dead_code)]
use crate::hip::{check, ss_searcher, DeviceSlice, DynamicHipSearcher};
use crate::Needle;
use std::os::raw::{c_int, c_void};

extern "C" {
    pub fn ss_count_device(s: *const ss_searcher, d_haystack: *const c_void, len: usize, hip_stream: *mut c_void, count: *mut u64) -> c_int;
    pub fn ss_count_device_async(s: *const ss_searcher, d_haystack: *const c_void, len: usize, hip_stream: *mut c_void, d_count: *mut u64) -> c_int;
    pub fn ss_find_all_device(s: *const ss_searcher, d_haystack: *const c_void, len: usize, hip_stream: *mut c_void, d_offsets: *mut u64,
                              capacity: u64, count: *mut u64) -> c_int;
}

/// Every (overlapping) occurrence - the shape of `memchr::memmem::find_iter` and `bytes.count`.  An empty needle occurs at
/// 0 ..= len.  The searcher must come from the matches library (a crate built with `hip-matches`).
pub trait FindAll {
    /// The number of occurrences in a device-resident haystack.
    fn count_in(&self, haystack: DeviceSlice, stream: *mut c_void) -> u64;
    /// The total count, and the leftmost `min(total, capacity)` offsets written to the device buffer `d_offsets` in ascending
    /// order (`d_offsets[capacity..]` is never written; capacity 0: count only, `d_offsets` may be null).
    fn find_all_in(&self, haystack: DeviceSlice, stream: *mut c_void, d_offsets: *mut u64, capacity: u64) -> u64;
}

impl<N: Needle> FindAll for DynamicHipSearcher<N> {
    fn count_in(&self, haystack: DeviceSlice, stream: *mut c_void) -> u64 {
        let mut count = 0u64;
        check(unsafe { ss_count_device(self.handle(), haystack.ptr, haystack.len, stream, &mut count) });
        count
    }
    fn find_all_in(&self, haystack: DeviceSlice, stream: *mut c_void, d_offsets: *mut u64, capacity: u64) -> u64 {
        let mut count = 0u64;
        check(unsafe { ss_find_all_device(self.handle(), haystack.ptr, haystack.len, stream, d_offsets, capacity, &mut count) });
        count
    }
}
