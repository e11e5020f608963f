// ss_bounded.hip - the every-occurrence and matching-lines calls for whole words and whole lines (include/sliceslice_hip_bounded.h).
// NOT in the other libraries: libsliceslice_hip_bounded.so holds the nocase library's objects plus this file, scan_inst_bounded.hip
// and scan_inst_bounded_nocase.hip.
//
// The host side is the models' own (matches_host.hpp, lines_host.hpp) with the bounded scans of bounded_kernels.hpp in place of
// launch_scan_all / launch_scan_lines and their mode word as the helpers' last argument.  check_how (bounded_how.hpp) checks `how` and the needle
// (not empty; no upper-case byte with SS_BOUND_NOCASE) and builds the mode word; n > len and a needle that holds the delimiter are
// settled by the models' code before any scan is launched.
#include "ss_internal.hpp"

#include "../../include/sliceslice_hip_bounded.h"
#include "bounded_how.hpp"
#include "bounded_launch.hpp"
#include "lines_host.hpp"
#include "matches_host.hpp"
#include "nocase_launch.hpp"

namespace ssh {
namespace {

ss::ScanAllFn scan_all_of(unsigned how) { return (how & SS_BOUND_NOCASE) ? ss::launch_scan_all_bounded_nocase : ss::launch_scan_all_bounded; }
ss::ScanLinesFn scan_lines_of(unsigned how) { return (how & SS_BOUND_NOCASE) ? ss::launch_scan_lines_bounded_nocase : ss::launch_scan_lines_bounded; }

}  // namespace
}  // namespace ssh

using namespace ssh;

extern "C" {

int ss_count_bounded_device(const ss_searcher *s, const void *d_haystack, size_t len, unsigned how, void *hip_stream, uint64_t *count)
{
    uint32_t bound = 0;
    if (int rc = check_how(s, how, false, 0, "ss_count_bounded_device", &bound)) return rc;
    return count_device_with(scan_all_of(how), s, d_haystack, len, hip_stream, count, bound);
}

int ss_count_bounded_device_async(const ss_searcher *s, const void *d_haystack, size_t len, unsigned how, void *hip_stream,
                                  uint64_t *d_count)
{
    uint32_t bound = 0;
    if (int rc = check_how(s, how, false, 0, "ss_count_bounded_device_async", &bound)) return rc;
    return count_device_async_with(scan_all_of(how), s, d_haystack, len, hip_stream, d_count, bound);
}

int ss_find_all_bounded_device(const ss_searcher *s, const void *d_haystack, size_t len, unsigned how, void *hip_stream,
                               uint64_t *d_offsets, uint64_t capacity, uint64_t *count)
{
    uint32_t bound = 0;
    if (int rc = check_how(s, how, false, 0, "ss_find_all_bounded_device", &bound)) return rc;
    return find_all_device_with(scan_all_of(how), s, d_haystack, len, hip_stream, d_offsets, capacity, count, bound);
}

int ss_count_lines_bounded_device(const ss_searcher *s, const void *d_haystack, size_t len, int delimiter, unsigned how,
                                  void *hip_stream, uint64_t *lines)
{
    uint32_t bound = 0;
    if (int rc = check_how(s, how, true, delimiter, "ss_count_lines_bounded_device", &bound)) return rc;
    return count_lines_device_with(scan_lines_of(how), s, d_haystack, len, delimiter, hip_stream, lines, bound);
}

int ss_count_lines_bounded_device_async(const ss_searcher *s, const void *d_haystack, size_t len, int delimiter, unsigned how,
                                        void *hip_stream, uint64_t *d_lines)
{
    uint32_t bound = 0;
    if (int rc = check_how(s, how, true, delimiter, "ss_count_lines_bounded_device_async", &bound)) return rc;
    return count_lines_device_async_with(scan_lines_of(how), "ss_count_lines_bounded_device_async", s, d_haystack, len, delimiter,
                                         hip_stream, d_lines, bound);
}

int ss_find_lines_bounded_device(const ss_searcher *s, const void *d_haystack, size_t len, int delimiter, unsigned how,
                                 void *hip_stream, uint64_t *d_begin, uint64_t *d_end, uint64_t *d_number, uint64_t capacity,
                                 uint64_t *lines)
{
    uint32_t bound = 0;
    if (int rc = check_how(s, how, true, delimiter, "ss_find_lines_bounded_device", &bound)) return rc;
    return find_lines_device_with(scan_lines_of(how), s, d_haystack, len, delimiter, hip_stream, d_begin, d_end, d_number, capacity,
                                  lines, bound);
}

}  // extern "C"
