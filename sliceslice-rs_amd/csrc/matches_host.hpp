// matches_host.hpp - the host side of the every-occurrence calls with the scan launcher as an argument (defined in ss_matches.hip):
// ss_count_device / _async and ss_find_all_device pass launch_scan_all, their case-folding forms (ss_nocase.hip) the folding twin.
// Everything else - argument checks, the empty needle, n > len, launch shape, scratch, prefix sum, the emit pass - is one code.
#pragma once
#include "matches_launch.hpp"

struct ss_searcher;

namespace ssh {

int count_device_with(ss::ScanAllFn scan, const ss_searcher *s, const void *d_haystack, size_t len, void *hip_stream, uint64_t *count);
int count_device_async_with(ss::ScanAllFn scan, const ss_searcher *s, const void *d_haystack, size_t len, void *hip_stream,
                            uint64_t *d_count);
int find_all_device_with(ss::ScanAllFn scan, const ss_searcher *s, const void *d_haystack, size_t len, void *hip_stream,
                         uint64_t *d_offsets, uint64_t capacity, uint64_t *count);

}  // namespace ssh
