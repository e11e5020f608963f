// src/hip_setmatches.rs - every occurrence of every needle of a compiled set, counted per needle and listed as (offset, rank) pairs
// in ONE pass over the haystack (include/sliceslice_hip_setmatches.h): an OPT-IN component gated by a feature of its own
// (`#[cfg(feature = "hip-setmatches")] pub mod hip_setmatches;`).  A crate built with that feature links
// libsliceslice_hip_setmatches.so - the needleset library's objects plus the occurrence scan - INSTEAD of libsliceslice_hip.so (and
// enables `hip-needleset` next to it: the sets are made there, and the library holds those entry points too).
//
// SOURCE ONLY, like src/hip.rs: never compiled here (no rustc); the `extern "C"` block is checked mechanically against
// include/sliceslice_hip_setmatches.h by tests/test_setmatches_cpu.py.
#![allow(non_camel_case_types, dead_code)]
use crate::hip::{check, DeviceSlice};
use crate::hip_needleset::{ss_needle_set, NeedleSet};
use std::os::raw::{c_int, c_uint, c_void};

extern "C" {
    pub fn ss_needle_set_ranks(set: *const ss_needle_set, ranks: *mut u32) -> c_int;
    pub fn ss_count_set_device(set: *const ss_needle_set, d_haystack: *const c_void, len: usize, how: c_uint, hip_stream: *mut c_void,
                               d_counts: *mut u64, total: *mut u64) -> c_int;
    pub fn ss_count_set_device_async(set: *const ss_needle_set, d_haystack: *const c_void, len: usize, how: c_uint, hip_stream: *mut c_void,
                                     d_counts: *mut u64, d_total: *mut u64) -> c_int;
    pub fn ss_find_all_set_device(set: *const ss_needle_set, d_haystack: *const c_void, len: usize, how: c_uint, hip_stream: *mut c_void,
                                  d_offsets: *mut u64, d_ranks: *mut u32, capacity: u64, total: *mut u64) -> c_int;
}

/// The occurrence calls of a set; `how` is 0 or SS_BOUND_WORD, | SS_BOUND_NOCASE iff the set folds.
pub trait SetMatches {
    fn raw_set(&self) -> *const ss_needle_set;

    /// The rank of every needle as given (`needles` entries): its position in the sorted, deduplicated order.
    fn ranks(&self, needles: usize) -> Vec<u32> {
        let mut out = vec![0u32; needles];
        check(unsafe { ss_needle_set_ranks(self.raw_set(), out.as_mut_ptr()) });
        out
    }

    /// The number of (offset, rank) pairs; `d_counts` (device, `distinct` words, or null) receives the count of every rank.
    fn count(&self, haystack: DeviceSlice, how: c_uint, stream: *mut c_void, d_counts: *mut u64) -> u64 {
        let mut total = 0u64;
        check(unsafe { ss_count_set_device(self.raw_set(), haystack.ptr, haystack.len, how, stream, d_counts, &mut total) });
        total
    }

    /// Enqueue only: counts and total land in device memory (either may be null, not both); capturable.
    fn count_async(&self, haystack: DeviceSlice, how: c_uint, stream: *mut c_void, d_counts: *mut u64, d_total: *mut u64) {
        check(unsafe { ss_count_set_device_async(self.raw_set(), haystack.ptr, haystack.len, how, stream, d_counts, d_total) });
    }

    /// The first `capacity` pairs ordered by offset, then by rank (either array may be null); returns the total.
    fn find_all(&self, haystack: DeviceSlice, how: c_uint, stream: *mut c_void, d_offsets: *mut u64, d_ranks: *mut u32, capacity: u64) -> u64 {
        let mut total = 0u64;
        check(unsafe {
            ss_find_all_set_device(self.raw_set(), haystack.ptr, haystack.len, how, stream, d_offsets, d_ranks, capacity, &mut total)
        });
        total
    }
}

impl SetMatches for NeedleSet {
    fn raw_set(&self) -> *const ss_needle_set {
        self.as_raw()
    }
}
