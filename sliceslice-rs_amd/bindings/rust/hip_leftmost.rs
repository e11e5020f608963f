// src/hip_leftmost.rs - the LEFTMOST-LONGEST, non-overlapping occurrences of a compiled needle set: how many, where, which needle,
// and the haystack with each of them replaced by its needle's own text (include/sliceslice_hip_leftmost.h; what
// `aho_corasick::MatchKind::LeftmostLongest` gives `find_iter` and `replace_all`, and `grep -o -F -f FILE` prints): an OPT-IN
// component gated by a feature of its own (`#[cfg(feature = "hip-leftmost")] pub mod hip_leftmost;`).  A crate built with that
// feature links libsliceslice_hip_leftmost.so - the output library's objects plus the selection and the set-replace kernels -
// INSTEAD of libsliceslice_hip.so (and enables `hip-needleset` and `hip-setmatches` next to it: the sets are made there, and the
// library holds those entry points too).
//
// SOURCE ONLY, like src/hip.rs: never compiled here (no rustc); the `extern "C"` block is checked mechanically against
// include/sliceslice_hip_leftmost.h by tests/test_leftmost_cpu.py.
#![allow(non_camel_case_types, dead_code)]
use crate::hip::{check, DeviceSlice};
use crate::hip_needleset::ss_needle_set;
use std::os::raw::{c_int, c_uint, c_void};

/// Entries per workgroup of the selection kernels.
pub const SS_LEFTMOST_BLOCK: u64 = 4096;

extern "C" {
    pub fn ss_select_leftmost_device(set: *const ss_needle_set, d_offsets: *const u64, d_lengths: *const u64, count: u64,
                                     hip_stream: *mut c_void, d_selected: *mut u64, d_which: *mut u64, capacity: u64,
                                     selected: *mut u64) -> c_int;
    pub fn ss_count_leftmost_set_device(set: *const ss_needle_set, d_haystack: *const c_void, len: usize, how: c_uint,
                                        hip_stream: *mut c_void, count: *mut u64) -> c_int;
    pub fn ss_find_all_leftmost_set_device(set: *const ss_needle_set, d_haystack: *const c_void, len: usize, how: c_uint,
                                           hip_stream: *mut c_void, d_offsets: *mut u64, d_ranks: *mut u32, capacity: u64,
                                           count: *mut u64) -> c_int;
    pub fn ss_replace_set_device(set: *const ss_needle_set, d_haystack: *const c_void, len: usize, how: c_uint,
                                 replacements: *const *const c_void, replacement_lens: *const usize, needles: u32,
                                 hip_stream: *mut c_void, d_out: *mut c_void, out_capacity: u64, out_len: *mut u64,
                                 count: *mut u64) -> c_int;
    pub fn ss_needle_set_lengths(set: *const ss_needle_set, lengths: *mut u64) -> c_int;
}

/// The size of the leftmost-longest selection over `count` entries (offset, length) in device memory; the leftmost `capacity`
/// selected offsets go to `d_selected` and their indices in the list to `d_which` (each may be null).  `set` names the device only.
pub fn select_leftmost(set: *const ss_needle_set, d_offsets: *const u64, d_lengths: *const u64, count: u64, stream: *mut c_void,
                       d_selected: *mut u64, d_which: *mut u64, capacity: u64) -> u64 {
    let mut selected = 0u64;
    check(unsafe { ss_select_leftmost_device(set, d_offsets, d_lengths, count, stream, d_selected, d_which, capacity, &mut selected) });
    selected
}

/// The number of selected occurrences; `how` is 0 or SS_BOUND_WORD, | SS_BOUND_NOCASE iff the set folds.
pub fn count_leftmost(set: *const ss_needle_set, haystack: DeviceSlice, how: c_uint, stream: *mut c_void) -> u64 {
    let mut count = 0u64;
    check(unsafe { ss_count_leftmost_set_device(set, haystack.ptr, haystack.len, how, stream, &mut count) });
    count
}

/// That number; the leftmost `capacity` selected offsets and the ranks of their needles go to the device arrays (each may be null).
pub fn find_all_leftmost(set: *const ss_needle_set, haystack: DeviceSlice, how: c_uint, stream: *mut c_void, d_offsets: *mut u64,
                         d_ranks: *mut u32, capacity: u64) -> u64 {
    let mut count = 0u64;
    check(unsafe { ss_find_all_leftmost_set_device(set, haystack.ptr, haystack.len, how, stream, d_offsets, d_ranks, capacity, &mut count) });
    count
}

/// (out_len, count) of the haystack with every selected occurrence replaced by the text of its needle (`replacements[k]` belongs to
/// needle k as given); the bytes are written to `d_out` when `out_capacity` holds them, nothing is written otherwise.
pub fn replace_set(set: *const ss_needle_set, haystack: DeviceSlice, how: c_uint, replacements: &[&[u8]], stream: *mut c_void,
                   d_out: *mut c_void, out_capacity: u64) -> (u64, u64) {
    let ptrs: Vec<*const c_void> = replacements.iter().map(|r| r.as_ptr() as *const c_void).collect();
    let lens: Vec<usize> = replacements.iter().map(|r| r.len()).collect();
    let (mut out_len, mut count) = (0u64, 0u64);
    check(unsafe {
        ss_replace_set_device(set, haystack.ptr, haystack.len, how, ptrs.as_ptr(), lens.as_ptr(), replacements.len() as u32, stream, d_out,
                              out_capacity, &mut out_len, &mut count)
    });
    (out_len, count)
}

/// The length of the needle of every rank (`distinct` entries).
pub fn set_lengths(set: *const ss_needle_set, distinct: usize) -> Vec<u64> {
    let mut out = vec![0u64; distinct];
    check(unsafe { ss_needle_set_lengths(set, out.as_mut_ptr()) });
    out
}
