// lines_host.hpp - the host side of the matching-lines calls with the scan launcher as an argument (defined in ss_lines.hip):
// ss_count_lines_device / _async and ss_find_lines_device pass launch_scan_lines, their case-folding forms (ss_nocase.hip) the
// folding twin.  `name` is the public function's, for the message that refuses a capturing stream; `bound` is handed to `scan` as it
// is (the whole-word / whole-line scans' mode word, ss_bounded.hip; 0 for every other scan).
#pragma once
#include "lines_launch.hpp"

struct ss_searcher;

namespace ssh {

int count_lines_device_with(ss::ScanLinesFn scan, const ss_searcher *s, const void *d_haystack, size_t len, int delimiter,
                            void *hip_stream, uint64_t *lines, uint32_t bound = 0);
int count_lines_device_async_with(ss::ScanLinesFn scan, const char *name, const ss_searcher *s, const void *d_haystack, size_t len,
                                  int delimiter, void *hip_stream, uint64_t *d_lines, uint32_t bound = 0);
int find_lines_device_with(ss::ScanLinesFn scan, const ss_searcher *s, const void *d_haystack, size_t len, int delimiter,
                           void *hip_stream, uint64_t *d_begin, uint64_t *d_end, uint64_t *d_number, uint64_t capacity, uint64_t *lines,
                           uint32_t bound = 0);

}  // namespace ssh
