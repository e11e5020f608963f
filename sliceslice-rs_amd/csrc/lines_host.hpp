// lines_host.hpp - the host side of the matching-lines calls with the scan launcher as an argument (defined in ss_lines.hip):
// ss_count_lines_device / _async and ss_find_lines_device pass launch_scan_lines, their case-folding forms (ss_nocase.hip) the
// folding twin.  `name` is the public function's, for the message that refuses a capturing stream; `bound` is handed to `scan` as it
// is (the whole-word / whole-line scans' mode word, ss_bounded.hip; 0 for every other scan).  `inverted`, when given, makes the call
// its inverse (include/sliceslice_hip_inverted.h, ss_inverted.hip): the lines WITHOUT a match, through the three launches it names.
#pragma once
#include "lines_launch.hpp"

struct ss_searcher;

namespace ssh {

// What an inverted call launches in place of the model's emit launches and behind its combine (inverted_launch.hpp).  Function
// pointers and not calls by name: the kernels exist in libsliceslice_hip_inverted.so only, ss_lines.hip in four libraries.
struct LinesInverted {
    ss::ScanLinesFn emit;                                                       // the scan's grid again, emit only
    hipError_t (*plain)(const ss::PlainArgs &pa, hipStream_t st);               // an edge part, emit only
    hipError_t (*total)(const ss::CombineArgs &ca, hipStream_t st);             // the total and an unterminated last line's record
};

int count_lines_device_with(ss::ScanLinesFn scan, const ss_searcher *s, const void *d_haystack, size_t len, int delimiter,
                            void *hip_stream, uint64_t *lines, uint32_t bound = 0, const LinesInverted *inverted = nullptr);
int count_lines_device_async_with(ss::ScanLinesFn scan, const char *name, const ss_searcher *s, const void *d_haystack, size_t len,
                                  int delimiter, void *hip_stream, uint64_t *d_lines, uint32_t bound = 0, const LinesInverted *inverted = nullptr);
int find_lines_device_with(ss::ScanLinesFn scan, const ss_searcher *s, const void *d_haystack, size_t len, int delimiter,
                           void *hip_stream, uint64_t *d_begin, uint64_t *d_end, uint64_t *d_number, uint64_t capacity, uint64_t *lines,
                           uint32_t bound = 0, const LinesInverted *inverted = nullptr);

}  // namespace ssh
