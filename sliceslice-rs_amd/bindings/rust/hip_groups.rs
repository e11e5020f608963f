// src/hip_groups.rs - equal tokens or lines grouped and counted on the device (`sort | uniq -c`, `awk '!seen[$0]++'`;
// include/sliceslice_hip_groups.h has the rule: the key of a range is its bytes, groups are numbered in order of their first
// member): an OPT-IN component gated by a feature of its own (`#[cfg(feature = "hip-groups")] pub mod hip_groups;`).  A crate built
// with that feature links libsliceslice_hip_groups.so - the fields library's objects plus the grouping - INSTEAD of
// libsliceslice_hip.so.
//
// SOURCE ONLY, like src/hip.rs: never compiled here (no rustc); the `extern "C"` block is checked mechanically against
// include/sliceslice_hip_groups.h by tests/test_groups_cpu.py.
#![allow(non_camel_case_types, dead_code)]
use crate::hip::{check, DeviceSlice};
use crate::hip_runs::ss_runs;
use std::os::raw::{c_int, c_uint, c_void};

/// Every key byte goes through the ASCII fold before it is hashed or compared.
pub const SS_GROUPS_NOCASE: c_uint = 1;
/// For tests: the hash is length & 3.
pub const SS_GROUPS_WEAK_HASH: c_uint = 2;
/// Ranges of a call: 2^32 - 2.
pub const SS_GROUPS_MAX_RANGES: u64 = 0xfffffffe;
/// Ranges per rank block.
pub const SS_GROUPS_BLOCK: usize = 4096;
/// The longest key one lane hashes and compares alone.
pub const SS_GROUPS_LANE_MAX: usize = 128;
/// The count kernel's workgroup-private LDS table.
pub const SS_GROUPS_LDS_BYTES: usize = 24576;

extern "C" {
    pub fn ss_group_ranges_device(d_haystack: *const c_void, len: usize, d_begin: *const u64, d_end: *const u64, n: u64, flags: c_uint,
                                  hip_stream: *mut c_void, d_first: *mut u64, d_count: *mut u64, capacity: u64, d_group: *mut u64,
                                  groups: *mut u64) -> c_int;
    pub fn ss_group_runs_device(runs: *const ss_runs, d_haystack: *const c_void, len: usize, flags: c_uint, hip_stream: *mut c_void,
                                d_begin: *mut u64, d_end: *mut u64, d_count: *mut u64, capacity: u64, groups: *mut u64,
                                tokens: *mut u64) -> c_int;
    pub fn ss_group_lines_device(d_haystack: *const c_void, len: usize, delimiter: c_int, flags: c_uint, hip_stream: *mut c_void,
                                 d_begin: *mut u64, d_end: *mut u64, d_number: *mut u64, d_count: *mut u64, capacity: u64,
                                 groups: *mut u64, lines: *mut u64) -> c_int;
    pub fn ss_groups_scratch_bytes(n: u64, bytes: *mut u64) -> c_int;
}

/// The number of groups; the first `capacity` (first, count) rows and all `n` group numbers go to the device arrays that are not null.
pub fn group_ranges(haystack: DeviceSlice, d_begin: *const u64, d_end: *const u64, n: u64, ignore_case: bool, stream: *mut c_void,
                    d_first: *mut u64, d_count: *mut u64, capacity: u64, d_group: *mut u64) -> u64 {
    let mut groups = 0u64;
    check(unsafe {
        ss_group_ranges_device(haystack.ptr, haystack.len, d_begin, d_end, n, if ignore_case { SS_GROUPS_NOCASE } else { 0 }, stream,
                               d_first, d_count, capacity, d_group, &mut groups)
    });
    groups
}

/// (groups, tokens): the runs of `runs` grouped in one call; d_begin / d_end are the first token of every group.
pub fn group_runs(runs: *const ss_runs, haystack: DeviceSlice, ignore_case: bool, stream: *mut c_void, d_begin: *mut u64, d_end: *mut u64,
                  d_count: *mut u64, capacity: u64) -> (u64, u64) {
    let (mut groups, mut tokens) = (0u64, 0u64);
    check(unsafe {
        ss_group_runs_device(runs, haystack.ptr, haystack.len, if ignore_case { SS_GROUPS_NOCASE } else { 0 }, stream, d_begin, d_end,
                             d_count, capacity, &mut groups, &mut tokens)
    });
    (groups, tokens)
}

/// (groups, lines): one row per distinct line in first-occurrence order.
pub fn group_lines(haystack: DeviceSlice, delimiter: u8, ignore_case: bool, stream: *mut c_void, d_begin: *mut u64, d_end: *mut u64,
                   d_number: *mut u64, d_count: *mut u64, capacity: u64) -> (u64, u64) {
    let (mut groups, mut lines) = (0u64, 0u64);
    check(unsafe {
        ss_group_lines_device(haystack.ptr, haystack.len, delimiter as c_int, if ignore_case { SS_GROUPS_NOCASE } else { 0 }, stream,
                              d_begin, d_end, d_number, d_count, capacity, &mut groups, &mut lines)
    });
    (groups, lines)
}

/// The temporary device memory a call over `n` ranges takes.
pub fn scratch_bytes(n: u64) -> u64 {
    let mut bytes = 0u64;
    check(unsafe { ss_groups_scratch_bytes(n, &mut bytes) });
    bytes
}
