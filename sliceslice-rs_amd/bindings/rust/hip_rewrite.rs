// src/hip_rewrite.rs - the selected runs of one byte class replaced or deleted on the device (`tr -d '\r'`, `tr -s ' '`,
// `sed -E 's/[0-9]+/N/g'`; include/sliceslice_hip_rewrite.h has the rule: every selected run becomes the replacement, everything
// else is copied in order, and a delimiter byte is never a member): an OPT-IN component gated by a feature of its own
// (`#[cfg(feature = "hip-rewrite")] pub mod hip_rewrite;`).  A crate built with that feature links libsliceslice_hip_rewrite.so -
// the runs library's objects plus the rewrite - INSTEAD of libsliceslice_hip.so.
//
// SOURCE ONLY, like src/hip.rs: never compiled here (no rustc); the `extern "C"` block is checked mechanically against
// include/sliceslice_hip_rewrite.h by tests/test_rewrite_cpu.py.
#![allow(non_camel_case_types, dead_code)]
use crate::hip::{check, DeviceSlice};
use crate::hip_runs::ss_runs;
use std::os::raw::{c_int, c_void};

/// The longest replacement.
pub const SS_REWRITE_MAX_TEXT: usize = 4096;

extern "C" {
    pub fn ss_replace_runs_device(runs: *const ss_runs, d_haystack: *const c_void, len: usize, delimiter: c_int,
                                  replacement: *const c_void, replacement_len: usize, hip_stream: *mut c_void, d_out: *mut c_void,
                                  out_capacity: u64, out_len: *mut u64, count: *mut u64) -> c_int;
}

/// (out_len, count).  `delimiter`: a byte that is never a member, or None.  A null `d_out` with capacity 0 sizes; nothing is written
/// where `out_capacity` is below the output's length.
pub fn replace_runs(runs: *const ss_runs, haystack: DeviceSlice, delimiter: Option<u8>, replacement: &[u8], stream: *mut c_void,
                    d_out: *mut c_void, out_capacity: u64) -> (u64, u64) {
    let (mut out_len, mut count) = (0u64, 0u64);
    check(unsafe {
        ss_replace_runs_device(runs, haystack.ptr, haystack.len, delimiter.map_or(-1, |b| b as c_int), replacement.as_ptr() as *const c_void,
                               replacement.len(), stream, d_out, out_capacity, &mut out_len, &mut count)
    });
    (out_len, count)
}
