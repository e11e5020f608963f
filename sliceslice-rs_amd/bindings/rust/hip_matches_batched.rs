// src/hip_matches_batched.rs - every occurrence for a BATCH of problems (include/sliceslice_hip_matches_batched.h): per-problem
// counts and per-problem offsets in CSR form, an OPT-IN component gated by a feature of its own
// (`#[cfg(feature = "hip-matches-batched")] pub mod hip_matches_batched;`).  A crate built with that feature links
// libsliceslice_hip_matches_batched.so - the matches library's objects plus the batched all-matches scan - INSTEAD of
// libsliceslice_hip.so / libsliceslice_hip_matches.so.
//
// SOURCE ONLY, like src/hip.rs: never compiled here (no rustc); the `extern "C"` block is checked mechanically against
// include/sliceslice_hip_matches_batched.h by tests/test_matches_batched_cpu.py.
#![allow(non_camel_case_types, dead_code)]
use crate::hip::check;
use std::os::raw::{c_int, c_void};

extern "C" {
    pub fn ss_count_batched(d_haystacks: *const c_void, d_hay_begin: *const u64, d_hay_end: *const u64, d_needles: *const c_void,
                            d_needle_begin: *const u64, d_needle_end: *const u64, count: usize, hip_stream: *mut c_void,
                            d_counts: *mut u64) -> c_int;
    pub fn ss_find_all_batched(d_haystacks: *const c_void, d_hay_begin: *const u64, d_hay_end: *const u64, d_needles: *const c_void,
                               d_needle_begin: *const u64, d_needle_end: *const u64, count: usize, hip_stream: *mut c_void,
                               d_counts: *mut u64, d_row_begin: *mut u64, d_offsets: *mut u64, capacity: u64, total: *mut u64) -> c_int;
}

/// `count` problems given as device-resident range arrays (`begin[i] .. end[i]` into the two blobs; ranges may alias).
#[derive(Clone, Copy)]
pub struct DeviceBatch {
    pub haystacks: *const c_void,
    pub hay_begin: *const u64,
    pub hay_end: *const u64,
    pub needles: *const c_void,
    pub needle_begin: *const u64,
    pub needle_end: *const u64,
    pub count: usize,
}

impl DeviceBatch {
    /// Enqueue only: `d_counts[i]` = (overlapping) occurrences of needle i in haystack i.
    pub fn count_into(&self, stream: *mut c_void, d_counts: *mut u64) {
        check(unsafe {
            ss_count_batched(self.haystacks, self.hay_begin, self.hay_end, self.needles, self.needle_begin, self.needle_end, self.count, stream,
                             d_counts)
        });
    }
    /// CSR: `d_row_begin` (count + 1 entries) and the leftmost `min(total, capacity)` offsets in (problem, offset) order; returns
    /// the total.  `d_counts` may be null; capacity 0: rows and counts only.
    pub fn find_all_into(&self, stream: *mut c_void, d_counts: *mut u64, d_row_begin: *mut u64, d_offsets: *mut u64, capacity: u64) -> u64 {
        let mut total = 0u64;
        check(unsafe {
            ss_find_all_batched(self.haystacks, self.hay_begin, self.hay_end, self.needles, self.needle_begin, self.needle_end, self.count,
                                stream, d_counts, d_row_begin, d_offsets, capacity, &mut total)
        });
        total
    }
}
