// src/hip_needleset.rs - the lines that match any of many needles, selected in ONE pass over the haystack
// (include/sliceslice_hip_needleset.h, grep -e A -e B / grep -f FILE): an OPT-IN component gated by a feature of its own
// (`#[cfg(feature = "hip-needleset")] pub mod hip_needleset;`).  A crate built with that feature links
// libsliceslice_hip_needleset.so - the anyof library's objects plus the set scan - INSTEAD of libsliceslice_hip.so (and may enable
// `hip-matches`, `hip-lines`, `hip-nocase`, `hip-bounded`, `hip-inverted`, `hip-context` and `hip-anyof` next to it: the library
// holds those entry points too).
//
// SOURCE ONLY, like src/hip.rs: never compiled here (no rustc); the `extern "C"` block is checked mechanically against
// include/sliceslice_hip_needleset.h by tests/test_needleset_cpu.py.
#![allow(non_camel_case_types, dead_code)]
use crate::hip::{check, DeviceSlice};
use crate::hip_lines::LineRecords;
use std::os::raw::{c_int, c_uint, c_void};

/// ss_needle_set_new flags: the needles are compared ignoring ASCII case.
pub const SS_SET_NOCASE: c_uint = 1;

#[repr(C)]
pub struct ss_needle_set {
    _private: [u8; 0],
}

/// What ss_needle_set_info reports: eight 64-bit words.
#[repr(C)]
#[derive(Clone, Copy, Default, Debug)]
pub struct ss_needle_set_stats {
    pub needles: u64,
    pub distinct: u64,
    pub blob_bytes: u64,
    pub one_byte: u64,
    pub two_byte: u64,
    pub prefix_keys: u64,
    pub largest_bucket: u64,
    pub fold: u64,
}

extern "C" {
    pub fn ss_needle_set_new(needles: *const *const c_void, lens: *const usize, count: u32, flags: c_uint, out: *mut *mut ss_needle_set) -> c_int;
    pub fn ss_needle_set_free(set: *mut ss_needle_set);
    pub fn ss_needle_set_info(set: *const ss_needle_set, stats: *mut ss_needle_set_stats) -> c_int;
    pub fn ss_count_lines_set_device(set: *const ss_needle_set, d_haystack: *const c_void, len: usize, delimiter: c_int, how: c_uint,
                                     hip_stream: *mut c_void, lines: *mut u64) -> c_int;
    pub fn ss_find_lines_set_device(set: *const ss_needle_set, d_haystack: *const c_void, len: usize, delimiter: c_int, how: c_uint,
                                    before: u64, after: u64, hip_stream: *mut c_void, d_begin: *mut u64, d_end: *mut u64,
                                    d_number: *mut u64, d_kind: *mut u8, capacity: u64, lines: *mut u64, selected: *mut u64) -> c_int;
}

/// A compiled set of needles on the current device.
pub struct NeedleSet {
    raw: *mut ss_needle_set,
}

impl NeedleSet {
    pub fn new(needles: &[&[u8]], ignore_case: bool) -> NeedleSet {
        let ptrs: Vec<*const c_void> = needles.iter().map(|n| n.as_ptr() as *const c_void).collect();
        let lens: Vec<usize> = needles.iter().map(|n| n.len()).collect();
        let mut raw = std::ptr::null_mut();
        check(unsafe {
            ss_needle_set_new(ptrs.as_ptr(), lens.as_ptr(), needles.len() as u32, if ignore_case { SS_SET_NOCASE } else { 0 }, &mut raw)
        });
        NeedleSet { raw }
    }

    /// The handle, for the calls of other modules that take a set (hip_setmatches.rs).
    pub fn as_raw(&self) -> *const ss_needle_set {
        self.raw
    }

    pub fn info(&self) -> ss_needle_set_stats {
        let mut stats = ss_needle_set_stats::default();
        check(unsafe { ss_needle_set_info(self.raw, &mut stats) });
        stats
    }

    /// The lines that match any needle under `how` (SS_BOUND_WORD, SS_BOUND_LINE, SS_CONTEXT_INVERT; SS_BOUND_NOCASE iff the set folds).
    pub fn count_lines(&self, haystack: DeviceSlice, delimiter: u8, how: c_uint, stream: *mut c_void) -> u64 {
        let mut lines = 0u64;
        check(unsafe { ss_count_lines_set_device(self.raw, haystack.ptr, haystack.len, delimiter as c_int, how, stream, &mut lines) });
        lines
    }

    /// (total, selected): the size of the output and the number of selected lines, as `hip_anyof::find_lines_anyof`.
    pub fn find_lines(&self, haystack: DeviceSlice, delimiter: u8, how: c_uint, before: u64, after: u64, stream: *mut c_void,
                      out: &LineRecords, d_kind: *mut u8) -> (u64, u64) {
        let (mut lines, mut selected) = (0u64, 0u64);
        check(unsafe {
            ss_find_lines_set_device(self.raw, haystack.ptr, haystack.len, delimiter as c_int, how, before, after, stream, out.d_begin,
                                     out.d_end, out.d_number, d_kind, out.capacity, &mut lines, &mut selected)
        });
        (lines, selected)
    }
}

impl Drop for NeedleSet {
    fn drop(&mut self) {
        unsafe { ss_needle_set_free(self.raw) }
    }
}
