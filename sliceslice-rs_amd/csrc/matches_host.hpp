// matches_host.hpp - the host side of the every-occurrence calls with the scan launcher as an argument (defined in ss_matches.hip):
// ss_count_device / _async and ss_find_all_device pass launch_scan_all, their case-folding forms (ss_nocase.hip) the folding twin.
// Everything else - argument checks, the empty needle, n > len, launch shape, scratch, prefix sum, the emit pass - is one code.
// The launch shape (plan_static) is ss_lines.hip's too.
#pragma once
#include "matches_launch.hpp"
#include "ss_internal.hpp"

namespace ssh {

// One launch of (searcher, haystack) outside the tuned search: the Problem (fill_problem, the searcher's own filter bytes) and the
// shape an untuned search takes - workgroups per CU guessed from the needle, one or two contiguous tiles per workgroup (ss_scan.hip:
// guess_workgroups_per_cu, launch_grid).  The census is neither started nor read.
struct StaticPlan {
    ss::Problem pr;
    ProblemShape ps;
    ss::Shape shape;
    int q = 0, mode = 0;
    bool one_byte = false;
    uint64_t ntiles = 0;
};
constexpr uint64_t kPiecesPerTile = (ss::kBlock / ss::kWave) * 4;       // at U = 4
int plan_static(const ss_searcher *s, PerDevice *pd, const void *d_hay, size_t len, StaticPlan *out);
// what every call checks first: the handle, the result pointer, the haystack
int check_common_args(const ss_searcher *s, const void *d_haystack, size_t len, const void *out);

// (`bound`: handed to `scan` as it is - the whole-word scans' mode word, ss_bounded.hip; 0 for every other scan)
int count_device_with(ss::ScanAllFn scan, const ss_searcher *s, const void *d_haystack, size_t len, void *hip_stream, uint64_t *count,
                      uint32_t bound = 0);
int count_device_async_with(ss::ScanAllFn scan, const ss_searcher *s, const void *d_haystack, size_t len, void *hip_stream,
                            uint64_t *d_count, uint32_t bound = 0);
int find_all_device_with(ss::ScanAllFn scan, const ss_searcher *s, const void *d_haystack, size_t len, void *hip_stream,
                         uint64_t *d_offsets, uint64_t capacity, uint64_t *count, uint32_t bound = 0);

}  // namespace ssh
