// ss_nocase.hip - the every-occurrence and matching-lines calls ignoring ASCII case (include/sliceslice_hip_nocase.h).  NOT in the
// other libraries: libsliceslice_hip_nocase.so holds the lines library's objects plus this file and scan_inst_nocase.hip.
//
// The host side is the models' own (matches_host.hpp, lines_host.hpp) with the case-folding scans of nocase_kernels.hpp in place of
// launch_scan_all / launch_scan_lines: the kernels fold every haystack byte they compare, the needle is lower case already - which
// is all this file checks, on the host copy of the needle.  The empty needle, n > len and a needle that holds the delimiter are
// settled by the models' code before any scan is launched; the delimiter is compared raw everywhere.
#include "ss_internal.hpp"

#include "../../include/sliceslice_hip_nocase.h"
#include "lines_host.hpp"
#include "matches_host.hpp"
#include "nocase_launch.hpp"

#include <algorithm>
#include <vector>

namespace ssh {
namespace {

inline bool is_upper(uint8_t b) { return b >= 'A' && b <= 'Z'; }

}  // namespace

// the kernels compare folded haystack bytes with the needle's bytes as they are (nocase_launch.hpp: ss_bounded.hip asks too)
int check_folded(const ss_searcher *s, const char *name)
{
    if (!s) return SS_OK;                           // (the models' argument checks name it)
    const auto end = s->needle.begin() + (long)s->n;
    const auto up = std::find_if(s->needle.begin(), end, is_upper);
    if (up == end) return SS_OK;
    return fail(SS_ERR_ARGUMENT, "%s: the needle holds the upper-case byte 0x%02x at index %zu; create the searcher with ss_searcher_new_nocase "
                                 "(or from a needle without 'A'..'Z')", name, (unsigned)*up, (size_t)(up - s->needle.begin()));
}

}  // namespace ssh

using namespace ssh;

extern "C" {

int ss_searcher_new_nocase(const uint8_t *needle, size_t n, ss_searcher **out)
{
    if (n && !needle) return fail(SS_ERR_ARGUMENT, "needle is NULL");
    std::vector<uint8_t> folded(needle, needle + n);
    for (uint8_t &b : folded)
        if (is_upper(b)) b |= 0x20;
    return ss_searcher_new(folded.data(), n, out);
}

int ss_count_nocase_device(const ss_searcher *s, const void *d_haystack, size_t len, void *hip_stream, uint64_t *count)
{
    if (int rc = check_folded(s, "ss_count_nocase_device")) return rc;
    return count_device_with(ss::launch_scan_all_nocase, s, d_haystack, len, hip_stream, count);
}

int ss_count_nocase_device_async(const ss_searcher *s, const void *d_haystack, size_t len, void *hip_stream, uint64_t *d_count)
{
    if (int rc = check_folded(s, "ss_count_nocase_device_async")) return rc;
    return count_device_async_with(ss::launch_scan_all_nocase, s, d_haystack, len, hip_stream, d_count);
}

int ss_find_all_nocase_device(const ss_searcher *s, const void *d_haystack, size_t len, void *hip_stream, uint64_t *d_offsets,
                              uint64_t capacity, uint64_t *count)
{
    if (int rc = check_folded(s, "ss_find_all_nocase_device")) return rc;
    return find_all_device_with(ss::launch_scan_all_nocase, s, d_haystack, len, hip_stream, d_offsets, capacity, count);
}

int ss_count_lines_nocase_device(const ss_searcher *s, const void *d_haystack, size_t len, int delimiter, void *hip_stream,
                                 uint64_t *lines)
{
    if (int rc = check_folded(s, "ss_count_lines_nocase_device")) return rc;
    return count_lines_device_with(ss::launch_scan_lines_nocase, s, d_haystack, len, delimiter, hip_stream, lines);
}

int ss_count_lines_nocase_device_async(const ss_searcher *s, const void *d_haystack, size_t len, int delimiter, void *hip_stream,
                                       uint64_t *d_lines)
{
    if (int rc = check_folded(s, "ss_count_lines_nocase_device_async")) return rc;
    return count_lines_device_async_with(ss::launch_scan_lines_nocase, "ss_count_lines_nocase_device_async", s, d_haystack, len, delimiter,
                                         hip_stream, d_lines);
}

int ss_find_lines_nocase_device(const ss_searcher *s, const void *d_haystack, size_t len, int delimiter, void *hip_stream,
                                uint64_t *d_begin, uint64_t *d_end, uint64_t *d_number, uint64_t capacity, uint64_t *lines)
{
    if (int rc = check_folded(s, "ss_find_lines_nocase_device")) return rc;
    return find_lines_device_with(ss::launch_scan_lines_nocase, s, d_haystack, len, delimiter, hip_stream, d_begin, d_end, d_number,
                                  capacity, lines);
}

}  // extern "C"
