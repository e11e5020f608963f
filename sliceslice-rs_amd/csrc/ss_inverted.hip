// ss_inverted.hip - the lines that do NOT match (include/sliceslice_hip_inverted.h): ss_count_lines_inverted_device / _async,
// ss_find_lines_inverted_device.  NOT in the other libraries: libsliceslice_hip_inverted.so holds the bounded library's objects plus
// this file, scan_inst_inverted.hip and scan_inst_inverted_nocase.hip.
//
// The host side is the model's own (lines_host.hpp) with the scan launcher that `how` selects - plain, folding, bounded, bounded
// and folding - for the sum pass, and a LinesInverted that names what runs instead of the model's emit launches and behind its
// combine (inverted_launch.hpp).  check_how (bounded_how.hpp) is the bounded calls' with `how` = 0 and SS_BOUND_NOCASE alone let
// through; scratch, the lease and the async release are the model's.
#include "ss_internal.hpp"

#include "../../include/sliceslice_hip_inverted.h"
#include "bounded_how.hpp"
#include "inverted_launch.hpp"
#include "lines_host.hpp"

namespace ssh {
namespace {

ss::ScanLinesFn scan_lines_of(unsigned how)
{
    const bool fold = (how & SS_BOUND_NOCASE) != 0;
    if (how & (SS_BOUND_WORD | SS_BOUND_LINE)) return fold ? ss::launch_scan_lines_bounded_nocase : ss::launch_scan_lines_bounded;
    return fold ? ss::launch_scan_lines_nocase : ss::launch_scan_lines;
}

const LinesInverted *inverted_of(unsigned how)
{
    static const LinesInverted plain = {ss::launch_emit_lines_inverted, ss::launch_lines_plain_inverted, ss::launch_lines_total_inverted};
    static const LinesInverted fold = {ss::launch_emit_lines_inverted_nocase, ss::launch_lines_plain_inverted, ss::launch_lines_total_inverted};
    return (how & SS_BOUND_NOCASE) ? &fold : &plain;
}

}  // namespace
}  // namespace ssh

using namespace ssh;

extern "C" {

int ss_count_lines_inverted_device(const ss_searcher *s, const void *d_haystack, size_t len, int delimiter, unsigned how,
                                   void *hip_stream, uint64_t *lines)
{
    uint32_t bound = 0;
    if (int rc = check_how(s, how, true, delimiter, "ss_count_lines_inverted_device", &bound, true)) return rc;
    return count_lines_device_with(scan_lines_of(how), s, d_haystack, len, delimiter, hip_stream, lines, bound, inverted_of(how));
}

int ss_count_lines_inverted_device_async(const ss_searcher *s, const void *d_haystack, size_t len, int delimiter, unsigned how,
                                         void *hip_stream, uint64_t *d_lines)
{
    uint32_t bound = 0;
    if (int rc = check_how(s, how, true, delimiter, "ss_count_lines_inverted_device_async", &bound, true)) return rc;
    return count_lines_device_async_with(scan_lines_of(how), "ss_count_lines_inverted_device_async", s, d_haystack, len, delimiter,
                                         hip_stream, d_lines, bound, inverted_of(how));
}

int ss_find_lines_inverted_device(const ss_searcher *s, const void *d_haystack, size_t len, int delimiter, unsigned how,
                                  void *hip_stream, uint64_t *d_begin, uint64_t *d_end, uint64_t *d_number, uint64_t capacity,
                                  uint64_t *lines)
{
    uint32_t bound = 0;
    if (int rc = check_how(s, how, true, delimiter, "ss_find_lines_inverted_device", &bound, true)) return rc;
    return find_lines_device_with(scan_lines_of(how), s, d_haystack, len, delimiter, hip_stream, d_begin, d_end, d_number, capacity,
                                  lines, bound, inverted_of(how));
}

}  // extern "C"
