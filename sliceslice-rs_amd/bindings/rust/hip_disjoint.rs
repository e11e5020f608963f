// src/hip_disjoint.rs - the NON-OVERLAPPING occurrences of a needle: how many, where, and the haystack with each of them replaced
// (include/sliceslice_hip_disjoint.h; what str::matches, memmem::find_iter and str::replace give): an OPT-IN component gated by a
// feature of its own (`#[cfg(feature = "hip-disjoint")] pub mod hip_disjoint;`).  A crate built with that feature links
// libsliceslice_hip_disjoint.so - the setmatches library's objects plus the selection and the replace kernels - INSTEAD of
// libsliceslice_hip.so (and enables `hip-bounded` next to it: the `how` bits are defined there, and the library holds those entry
// points too).
//
// SOURCE ONLY, like src/hip.rs: never compiled here (no rustc); the `extern "C"` block is checked mechanically against
// include/sliceslice_hip_disjoint.h by tests/test_disjoint_cpu.py.
#![allow(non_camel_case_types, dead_code)]
use crate::hip::{check, ss_searcher, DeviceSlice};
use crate::hip_bounded::{SS_BOUND_NOCASE, SS_BOUND_WORD};
use std::os::raw::{c_int, c_uint, c_void};

/// Offsets per workgroup of the selection kernels.
pub const SS_DISJOINT_BLOCK: u64 = 4096;

extern "C" {
    pub fn ss_select_disjoint_device(s: *const ss_searcher, d_offsets: *const u64, count: u64, n: u64, hip_stream: *mut c_void,
                                     d_selected: *mut u64, capacity: u64, selected: *mut u64) -> c_int;
    pub fn ss_count_disjoint_device(s: *const ss_searcher, d_haystack: *const c_void, len: usize, how: c_uint, hip_stream: *mut c_void,
                                    count: *mut u64) -> c_int;
    pub fn ss_find_all_disjoint_device(s: *const ss_searcher, d_haystack: *const c_void, len: usize, how: c_uint, hip_stream: *mut c_void,
                                       d_offsets: *mut u64, capacity: u64, count: *mut u64) -> c_int;
    pub fn ss_replace_device(s: *const ss_searcher, d_haystack: *const c_void, len: usize, how: c_uint, replacement: *const c_void,
                             replacement_len: usize, hip_stream: *mut c_void, d_out: *mut c_void, out_capacity: u64, out_len: *mut u64,
                             count: *mut u64) -> c_int;
}

fn how(whole_word: bool, nocase: bool) -> c_uint {
    (if whole_word { SS_BOUND_WORD } else { 0 }) | (if nocase { SS_BOUND_NOCASE } else { 0 })
}

/// The greedy selection over `count` strictly ascending offsets in device memory of occurrences of length `n`: the first, and after a
/// selected p the first at or beyond p + n.  The leftmost `min(total, capacity)` go to `d_selected` (may be null); `s` names the
/// device only.
pub fn select_disjoint(s: *const ss_searcher, d_offsets: *const u64, count: u64, n: u64, stream: *mut c_void, d_selected: *mut u64,
                       capacity: u64) -> u64 {
    let mut selected = 0u64;
    check(unsafe { ss_select_disjoint_device(s, d_offsets, count, n, stream, d_selected, capacity, &mut selected) });
    selected
}

/// The number of non-overlapping occurrences (`nocase` needs a needle without 'A'..'Z').
pub fn count_disjoint(s: *const ss_searcher, haystack: DeviceSlice, whole_word: bool, nocase: bool, stream: *mut c_void) -> u64 {
    let mut count = 0u64;
    check(unsafe { ss_count_disjoint_device(s, haystack.ptr, haystack.len, how(whole_word, nocase), stream, &mut count) });
    count
}

/// Their leftmost `min(count, capacity)` offsets, ascending, into `d_offsets`; returns the count.
pub fn find_all_disjoint(s: *const ss_searcher, haystack: DeviceSlice, whole_word: bool, nocase: bool, stream: *mut c_void,
                         d_offsets: *mut u64, capacity: u64) -> u64 {
    let mut count = 0u64;
    check(unsafe {
        ss_find_all_disjoint_device(s, haystack.ptr, haystack.len, how(whole_word, nocase), stream, d_offsets, capacity, &mut count)
    });
    count
}

/// (out_len, count): the length of the haystack with every such occurrence replaced by `replacement`, and their number.  The bytes
/// are written to `d_out` when `out_capacity >= out_len`; nothing is written otherwise.
pub fn replace(s: *const ss_searcher, haystack: DeviceSlice, whole_word: bool, nocase: bool, replacement: &[u8], stream: *mut c_void,
               d_out: *mut c_void, out_capacity: u64) -> (u64, u64) {
    let (mut out_len, mut count) = (0u64, 0u64);
    check(unsafe {
        ss_replace_device(s, haystack.ptr, haystack.len, how(whole_word, nocase), replacement.as_ptr() as *const c_void, replacement.len(),
                          stream, d_out, out_capacity, &mut out_len, &mut count)
    });
    (out_len, count)
}
