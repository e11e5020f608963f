// src/hip_fields.rs - fields first .. last of every line, located on the device (`cut -d, -f3`, `awk '{print $2}'`;
// include/sliceslice_hip_fields.h has the rule: EACH separator ends a field, or runs of separators MERGE; a line with n fields is
// selected when n >= first; the delimiter is never a separator): an OPT-IN component gated by a feature of its own
// (`#[cfg(feature = "hip-fields")] pub mod hip_fields;`).  A crate built with that feature links libsliceslice_hip_fields.so -
// the rewrite library's objects plus the field scan - INSTEAD of libsliceslice_hip.so.
//
// SOURCE ONLY, like src/hip.rs: never compiled here (no rustc); the `extern "C"` block is checked mechanically against
// include/sliceslice_hip_fields.h by tests/test_fields_cpu.py.
#![allow(non_camel_case_types, dead_code)]
use crate::hip::{check, DeviceSlice};
use std::os::raw::{c_char, c_int, c_uint, c_void};

/// ss_fields_new modes: every separator ends a field (cut) / the fields are the runs between separators (awk).
pub const SS_FIELDS_EACH: c_int = 0;
pub const SS_FIELDS_MERGE: c_int = 1;
/// ss_fields_new flag: an empty record for every line that is not selected.
pub const SS_FIELDS_KEEP_SHORT: c_uint = 1;
/// Workgroup summaries per step of the carry kernel.
pub const SS_FIELDS_CARRY_CHUNK: usize = 256;

#[repr(C)]
pub struct ss_fields {
    _private: [u8; 0],
}

#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct ss_fields_stats {
    pub mode: u64,
    pub first: u64,
    pub last: u64,
    pub flags: u64,
    pub members: u64,
    pub accepts_delimiter: u64,
}

extern "C" {
    pub fn ss_fields_new(set: *const u64, mode: c_int, first: u64, last: u64, flags: c_uint, fields: *mut *mut ss_fields) -> c_int;
    pub fn ss_fields_free(fields: *mut ss_fields);
    pub fn ss_fields_info(fields: *const ss_fields, delimiter: c_int, stats: *mut ss_fields_stats) -> c_int;
    pub fn ss_fields_parse(text: *const c_char, first: *mut u64, last: *mut u64) -> c_int;
    pub fn ss_count_fields_device(fields: *const ss_fields, d_haystack: *const c_void, len: usize, delimiter: c_int,
                                  hip_stream: *mut c_void, lines_selected: *mut u64, lines_total: *mut u64) -> c_int;
    pub fn ss_find_fields_device(fields: *const ss_fields, d_haystack: *const c_void, len: usize, delimiter: c_int,
                                 hip_stream: *mut c_void, d_begin: *mut u64, d_end: *mut u64, d_number: *mut u64, capacity: u64,
                                 total: *mut u64) -> c_int;
}

/// Fields `first .. last` (last 0: to the line's end) of every line, split at the members of `set`.
pub struct FieldSelector {
    handle: *mut ss_fields,
}

impl FieldSelector {
    pub fn new(set: &[u64; 4], merge: bool, first: u64, last: u64, keep_short: bool) -> Self {
        let mut handle = std::ptr::null_mut();
        check(unsafe {
            ss_fields_new(set.as_ptr(), if merge { SS_FIELDS_MERGE } else { SS_FIELDS_EACH }, first, last,
                          if keep_short { SS_FIELDS_KEEP_SHORT } else { 0 }, &mut handle)
        });
        FieldSelector { handle }
    }

    /// (lines selected, lines in all)
    pub fn count(&self, haystack: DeviceSlice, delimiter: u8, stream: *mut c_void) -> (u64, u64) {
        let (mut selected, mut total) = (0u64, 0u64);
        check(unsafe { ss_count_fields_device(self.handle, haystack.ptr, haystack.len, delimiter as c_int, stream, &mut selected, &mut total) });
        (selected, total)
    }

    /// The total; the first `capacity` records go to the device arrays that are not null.
    pub fn find(&self, haystack: DeviceSlice, delimiter: u8, stream: *mut c_void, d_begin: *mut u64, d_end: *mut u64, d_number: *mut u64,
                capacity: u64) -> u64 {
        let mut total = 0u64;
        check(unsafe {
            ss_find_fields_device(self.handle, haystack.ptr, haystack.len, delimiter as c_int, stream, d_begin, d_end, d_number, capacity, &mut total)
        });
        total
    }
}

impl Drop for FieldSelector {
    fn drop(&mut self) {
        unsafe { ss_fields_free(self.handle) }
    }
}
