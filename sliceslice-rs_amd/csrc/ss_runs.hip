// ss_runs.hip - the maximal runs of one byte class, counted and listed in ONE pass over the haystack
// (include/sliceslice_hip_runs.h has THE RULE and the language): ss_runs_new / _free / _info, ss_runs_parse,
// ss_count_runs_device / _async, ss_find_all_runs_device, ss_count_lines_runs_device and ss_find_lines_runs_device.  NOT in the other
// libraries: libsliceslice_hip_runs.so holds the classes library's objects plus this file.
//
// A handle is host memory alone: the set, its ranges' constants and its bitmap travel in the kernels' argument block, so no call
// allocates device memory for the pattern.  The line calls are ss_masked.hip's, launch for launch, with the run kernel in place of
// the masked one.
#include "ss_internal.hpp"

#include "../../include/sliceslice_hip_runs.h"
#include "matches_scratch.hpp"
#include "runs_handle.hpp"
#include "runs_host.hpp"
#include "runs_kernels.hpp"

#include <new>

namespace ss {

hipError_t launch_runs_all(const RunsArgs &a, int mode, hipStream_t st)
{
    const dim3 grid((unsigned)((a.m.ntiles + kSetTiles - 1) / kSetTiles)), block(kBlock);
    if (mode == kRunsCount) hipLaunchKernelGGL((runs_all_kernel<kRunsCount>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((runs_all_kernel<kRunsEmit>), grid, block, 0, st, a);
    return hipGetLastError();
}

hipError_t launch_runs_lines(const RunsArgs &a, int mode, hipStream_t st)
{
    const dim3 grid((unsigned)((a.m.ntiles + kSetTiles - 1) / kSetTiles)), block(kBlock);
    if (mode == kMaskedSum) hipLaunchKernelGGL((runs_lines_kernel<kMaskedSum>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((runs_lines_kernel<kMaskedLineEmit>), grid, block, 0, st, a);
    return hipGetLastError();
}

}  // namespace ss

namespace ssh {
namespace {

// Both line calls.  `find`: records are wanted (else the four output arguments are unused).
int lines_runs(const char *name, bool find, const ss_runs *p, const void *d_haystack, size_t len, int delimiter, void *hip_stream,
               uint64_t *d_begin, uint64_t *d_end, uint64_t *d_number, uint64_t capacity, uint64_t *lines)
{
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    if (!lines) return fail(SS_ERR_ARGUMENT, "%s: lines is NULL", name);
    if (delimiter < 0 || delimiter > 255) return fail(SS_ERR_ARGUMENT, "delimiter %d is not a byte (0 .. 255)", delimiter);
    ss::RunsArgs ra;
    if (int rc = runs_args(name, p, d_haystack, len, true, st, &ra)) return rc;
    if (len == 0) {
        *lines = 0;
        return SS_OK;
    }
    ss::MaskedArgs &a = ra.m;
    ra.bits[delimiter >> 5] &= ~(1u << (delimiter & 31));                       // the delimiter is never a member
    const uint64_t parts = (a.ntiles + ss::kSetTiles - 1) / ss::kSetTiles;
    const uint64_t chunks = (parts + ss::kLineChunk - 1) / ss::kLineChunk;
    // [total, 32 bytes][LineSum x parts][LinePre x parts][LineSum x chunks][LinePre x chunks], as ss_masked.hip lays it out
    ScratchLease lease;
    if (int rc = take_scratch(p->dev, 32 + (parts + chunks) * (sizeof(ss::LineSum) + sizeof(ss::LinePre)), &lease.sc, st)) return rc;
    uint64_t *d_total = reinterpret_cast<uint64_t *>(lease.sc.d);
    ss::LineSum *sum = reinterpret_cast<ss::LineSum *>(lease.sc.d + 32);
    ss::LinePre *pre = reinterpret_cast<ss::LinePre *>(sum + parts);
    ss::LineSum *csum = reinterpret_cast<ss::LineSum *>(pre + parts);
    ss::LinePre *cpre = reinterpret_cast<ss::LinePre *>(csum + chunks);
    a.sum = sum;
    a.pre = pre;
    a.delim = (uint32_t)delimiter;
    HIP_TRY(ss::launch_runs_lines(ra, ss::kMaskedSum, st));
    HIP_TRY(ss::launch_lines_chunks(sum, parts, csum, cpre, pre, false, st));
    const bool emit = find && capacity != 0 && (d_begin || d_end || d_number);
    const ss::CombineArgs cb = {csum, chunks, cpre, d_total, nullptr, len, emit ? d_begin : nullptr, emit ? d_end : nullptr,
                                emit ? d_number : nullptr, emit ? capacity : 0};
    HIP_TRY(ss::launch_lines_combine(cb, st));
    if (emit) {
        HIP_TRY(ss::launch_lines_chunks(sum, parts, csum, cpre, pre, true, st));
        a.begin = d_begin;
        a.end = d_end;
        a.number = d_number;
        a.capacity = capacity;
        HIP_TRY(ss::launch_runs_lines(ra, ss::kMaskedLineEmit, st));
    }
    HIP_TRY(hipMemcpyAsync(lease.sc.h, d_total, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    lease.done = true;
    *lines = *lease.sc.h;
    return SS_OK;
}

}  // namespace
}  // namespace ssh

using namespace ssh;

extern "C" {

int ss_runs_parse(const char *text, int ignore_case, uint64_t *set, uint64_t *min_len, uint64_t *max_len)
{
    if (!text || !set || !min_len || !max_len) return fail(SS_ERR_ARGUMENT, "ss_runs_parse: NULL argument");
    classes::ParseError err = {0, nullptr};
    if (!runs::parse_runs(text, ignore_case != 0, set, min_len, max_len, &err))
        return fail(SS_ERR_ARGUMENT, "ss_runs_parse: column %zu: %s", err.column, err.what);
    return SS_OK;
}

int ss_runs_new(const uint64_t *set, uint64_t min_len, uint64_t max_len, unsigned flags, ss_runs **out)
{
    if (!out || !set) return fail(SS_ERR_ARGUMENT, "ss_runs_new: NULL argument");
    if (classes::set_size(set) == 0) return fail(SS_ERR_ARGUMENT, "ss_runs_new: the set is empty");
    if (const char *why = runs::check_lengths(min_len, max_len)) return fail(SS_ERR_ARGUMENT, "ss_runs_new: %s", why);
    if (flags & ~SS_RUNS_BITMAP) return fail(SS_ERR_ARGUMENT, "ss_runs_new: unknown flag bits 0x%x", flags & ~SS_RUNS_BITMAP);
    ss_runs *p = new (std::nothrow) ss_runs;
    if (!p) return fail(SS_ERR_NOMEM, "ss_runs_new: out of memory");
    for (int k = 0; k < 4; ++k) p->set[k] = set[k];
    p->min_len = min_len;
    p->max_len = max_len;
    uint8_t lo[ss::kRunsMaxRanges] = {0, 0, 0, 0}, hi[ss::kRunsMaxRanges] = {0, 0, 0, 0};
    p->nranges_all = ss::runs_ranges(set, lo, hi, ss::kRunsMaxRanges);
    p->path = (flags & SS_RUNS_BITMAP) || p->nranges_all > (uint32_t)ss::kRunsMaxRanges ? 1u : 0u;
    for (int r = 0; r < ss::kRunsMaxRanges; ++r) p->rg[r] = ss::runs_range(lo[r], hi[r]);
    const hipError_t e = hipGetDevice(&p->dev);
    if (e != hipSuccess) {
        delete p;
        return fail(SS_ERR_HIP, "ss_runs_new: %s", hipGetErrorString(e));
    }
    *out = p;
    return SS_OK;
}

void ss_runs_free(ss_runs *p) { delete p; }

int ss_runs_info(const ss_runs *p, int delimiter, ss_runs_stats *stats)
{
    if (!p || !stats) return fail(SS_ERR_ARGUMENT, "ss_runs_info: NULL argument");
    if (delimiter > 255) return fail(SS_ERR_ARGUMENT, "delimiter %d is not a byte (0 .. 255)", delimiter);
    const ss_runs_stats s = {p->min_len, p->max_len, classes::set_size(p->set), p->nranges_all, p->path,
                             delimiter >= 0 && classes::set_has(p->set, (unsigned)delimiter) ? 1u : 0u};
    *stats = s;
    return SS_OK;
}

int ss_count_runs_device_async(const ss_runs *p, const void *d_haystack, size_t len, void *hip_stream, uint64_t *d_count)
{
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    if (!d_count) return fail(SS_ERR_ARGUMENT, "ss_count_runs_device_async: d_count is NULL");
    ss::RunsArgs ra;
    if (int rc = runs_args("ss_count_runs_device_async", p, d_haystack, len, false, st, &ra)) return rc;
    HIP_TRY(hipMemsetAsync(d_count, 0, sizeof(uint64_t), st));
    if (len == 0) return SS_OK;
    ra.m.total = d_count;
    HIP_TRY(ss::launch_runs_all(ra, ss::kRunsCount, st));
    return SS_OK;
}

int ss_count_runs_device(const ss_runs *p, const void *d_haystack, size_t len, void *hip_stream, uint64_t *count)
{
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    if (!count) return fail(SS_ERR_ARGUMENT, "ss_count_runs_device: count is NULL");
    ss::RunsArgs ra;
    if (int rc = runs_args("ss_count_runs_device", p, d_haystack, len, true, st, &ra)) return rc;
    if (len == 0) {
        *count = 0;
        return SS_OK;
    }
    ScratchLease lease;
    if (int rc = take_scratch(p->dev, sizeof(uint64_t), &lease.sc, st)) return rc;
    ra.m.total = reinterpret_cast<uint64_t *>(lease.sc.d);
    HIP_TRY(hipMemsetAsync(ra.m.total, 0, sizeof(uint64_t), st));
    HIP_TRY(ss::launch_runs_all(ra, ss::kRunsCount, st));
    HIP_TRY(hipMemcpyAsync(lease.sc.h, ra.m.total, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    lease.done = true;
    *count = *lease.sc.h;
    return SS_OK;
}

int ss_find_all_runs_device(const ss_runs *p, const void *d_haystack, size_t len, void *hip_stream, uint64_t *d_begin, uint64_t *d_end,
                            uint64_t capacity, uint64_t *total)
{
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    if (!total) return fail(SS_ERR_ARGUMENT, "ss_find_all_runs_device: total is NULL");
    if (capacity && !d_begin && !d_end)
        return fail(SS_ERR_ARGUMENT, "ss_find_all_runs_device: both offset arrays are NULL with a capacity of %llu", (unsigned long long)capacity);
    ss::RunsArgs ra;
    if (int rc = runs_args("ss_find_all_runs_device", p, d_haystack, len, true, st, &ra)) return rc;
    if (len == 0) {
        *total = 0;
        return SS_OK;
    }
    ss::MaskedArgs &a = ra.m;
    const uint64_t parts = (a.ntiles + ss::kSetTiles - 1) / ss::kSetTiles;
    // [total of begins u64][total of ends u64][pad to 32][begins, ends, rank of begins, rank of ends: u64 x parts each]
    ScratchLease lease;
    if (int rc = take_scratch(p->dev, 32 + parts * 32, &lease.sc, st)) return rc;
    uint64_t *d_total = reinterpret_cast<uint64_t *>(lease.sc.d);
    uint64_t *wg_b = d_total + 4, *wg_e = wg_b + parts, *rank_b = wg_e + parts, *rank_e = rank_b + parts;
    ra.wg_b = wg_b;
    ra.wg_e = wg_e;
    HIP_TRY(ss::launch_runs_all(ra, ss::kRunsCount, st));
    HIP_TRY(ss::launch_set_prefix(wg_b, parts, rank_b, d_total, st));
    HIP_TRY(ss::launch_set_prefix(wg_e, parts, rank_e, d_total + 1, st));
    if (capacity != 0) {
        ra.rank_b = rank_b;
        ra.rank_e = rank_e;
        ra.out_b = d_begin;
        ra.out_e = d_end;
        a.capacity = capacity;
        HIP_TRY(ss::launch_runs_all(ra, ss::kRunsEmit, st));
    }
    HIP_TRY(hipMemcpyAsync(lease.sc.h, d_total, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    lease.done = true;
    *total = *lease.sc.h;
    return SS_OK;
}

int ss_count_lines_runs_device(const ss_runs *p, const void *d_haystack, size_t len, int delimiter, void *hip_stream, uint64_t *lines)
{
    return lines_runs("ss_count_lines_runs_device", false, p, d_haystack, len, delimiter, hip_stream, nullptr, nullptr, nullptr, 0, lines);
}

int ss_find_lines_runs_device(const ss_runs *p, const void *d_haystack, size_t len, int delimiter, void *hip_stream, uint64_t *d_begin,
                              uint64_t *d_end, uint64_t *d_number, uint64_t capacity, uint64_t *lines)
{
    return lines_runs("ss_find_lines_runs_device", true, p, d_haystack, len, delimiter, hip_stream, d_begin, d_end, d_number, capacity, lines);
}

}  // extern "C"
