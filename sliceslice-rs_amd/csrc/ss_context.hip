// ss_context.hip - matching lines with their context lines (include/sliceslice_hip_context.h): ss_lines_around_device and
// ss_find_lines_context_device.  NOT in the other libraries: libsliceslice_hip_context.so holds the inverted library's objects plus
// this file.
//
// ss_lines_around_device is the primitive: a line index of the view at streaming rate (context_census_kernel, one 8-byte count per
// part of SS_CONTEXT_PART_BYTES, and their prefix), the lines every entry of the caller's numbers owns (context_ranges.hpp) with
// their prefix, and - when records are wanted - the fill of number and kind and the select pass, which reads again only the parts
// that hold an end or a beginning of an output line below the capacity.  ss_find_lines_context_device counts its model's lines,
// lets the model's record call write their numbers into temporary device memory and hands them to the primitive; it calls the
// models through their public entry points, so every refusal is theirs.
#include "ss_internal.hpp"

#include "../../include/sliceslice_hip_context.h"
#include "context_kernels.hpp"
#include "matches_host.hpp"
#include "matches_scratch.hpp"

namespace ss {

hipError_t launch_context_census(const CtxArgs &ca, hipStream_t st)
{
    hipLaunchKernelGGL(context_census_kernel, dim3((unsigned)ca.parts), dim3(kBlock), 0, st, ca);
    return hipGetLastError();
}

hipError_t launch_context_part_prefix(const CtxArgs &ca, hipStream_t st)
{
    hipLaunchKernelGGL(prefix_kernel<uint64_t>, dim3(1), dim3(kPrefixThreads), 0, st, (const uint64_t *)ca.cnt, ca.parts, ca.pre, ca.ndelim);
    return hipGetLastError();
}

hipError_t launch_context_ranges(const CtxArgs &ca, hipStream_t st)
{
    hipLaunchKernelGGL(context_ranges_kernel, dim3((unsigned)((ca.count + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, ca);
    return hipGetLastError();
}

hipError_t launch_context_block_prefix(const CtxArgs &ca, hipStream_t st)
{
    hipLaunchKernelGGL(prefix_kernel<uint64_t>, dim3(1), dim3(kPrefixThreads), 0, st, (const uint64_t *)ca.bsum, (ca.count + kBlock - 1) / kBlock,
                       ca.bpre, ca.total);
    return hipGetLastError();
}

// The size of the output is known on the device only: a grid-stride loop over the slots below min(total, capacity), from a grid that
// fills the device (eight workgroups per CU) or covers the capacity, whichever is smaller.
hipError_t launch_context_fill(const CtxArgs &ca, int cus, hipStream_t st)
{
    const uint64_t want = (ca.capacity + kBlock - 1) / kBlock, most = (uint64_t)(cus > 0 ? cus : 256) * 8;
    hipLaunchKernelGGL(context_fill_kernel, dim3((unsigned)(want < most ? want : most)), dim3(kBlock), 0, st, ca);
    return hipGetLastError();
}

hipError_t launch_context_select(const CtxArgs &ca, hipStream_t st)
{
    hipLaunchKernelGGL(context_select_kernel, dim3((unsigned)ca.parts), dim3(kBlock), 0, st, ca);
    return hipGetLastError();
}

}  // namespace ss

namespace ssh {
namespace {

constexpr uint64_t kGridMax = 0x7fffffffull;

int check_context_args(const ss_searcher *s, const void *d_haystack, size_t len, int delimiter, const void *out, const char *name,
                       hipStream_t st)
{
    if (int rc = check_common_args(s, d_haystack, len, out)) return rc;
    if (delimiter < 0 || delimiter > 255) return fail(SS_ERR_ARGUMENT, "delimiter %d is not a byte (0 .. 255)", delimiter);
    if (stream_is_capturing(st))
        return fail(SS_ERR_ARGUMENT, "%s waits for its stream and cannot be captured into a hipGraph", name);
    return SS_OK;
}

// [total, ndelim: 32 bytes][cnt x parts][pre x parts][bsum x blocks][bpre x blocks][first x count]
int lines_around(const ss_searcher *s, const void *d_haystack, size_t len, int delimiter, const uint64_t *d_numbers, uint64_t count,
                 uint64_t before, uint64_t after, hipStream_t st, uint64_t *d_begin, uint64_t *d_end, uint64_t *d_number, uint8_t *d_kind,
                 uint64_t capacity, uint64_t *lines)
{
    if (count != 0 && len != 0 && !d_numbers)
        return fail(SS_ERR_ARGUMENT, "ss_lines_around_device: d_numbers is NULL and count is %llu", (unsigned long long)count);
    *lines = 0;
    if (count == 0 || len == 0) return SS_OK;
    const uint64_t mis = (uint64_t)(reinterpret_cast<uintptr_t>(d_haystack) & 15);
    ss::CtxArgs ca = {};
    ca.base = static_cast<const uint8_t *>(d_haystack) - mis;
    ca.lo = mis;
    ca.hi = mis + len;
    ca.parts = (ca.hi + SS_CONTEXT_PART_BYTES - 1) / SS_CONTEXT_PART_BYTES;
    const uint64_t blocks = (count + ss::kBlock - 1) / ss::kBlock;
    if (ca.parts > kGridMax)
        return fail(SS_ERR_ARGUMENT, "a haystack of %zu bytes needs %llu parts of %u bytes; a grid holds 2^31 - 1", len,
                    (unsigned long long)ca.parts, (unsigned)SS_CONTEXT_PART_BYTES);
    if (blocks > kGridMax)
        return fail(SS_ERR_ARGUMENT, "%llu line numbers need %llu workgroups; a grid holds 2^31 - 1", (unsigned long long)count,
                    (unsigned long long)blocks);
    PerDevice *pd = nullptr;
    if (int rc = get_per_device(s, &pd)) return rc;
    ScratchLease lease;
    if (int rc = take_scratch(pd->dev, 32 + (2 * ca.parts + 2 * blocks + count) * sizeof(uint64_t), &lease.sc, st)) return rc;
    uint64_t *w = reinterpret_cast<uint64_t *>(lease.sc.d);
    ca.total = w;
    ca.ndelim = w + 1;
    ca.cnt = w + 4;
    ca.pre = ca.cnt + ca.parts;
    ca.bsum = ca.pre + ca.parts;
    ca.bpre = ca.bsum + blocks;
    ca.first = ca.bpre + blocks;
    ca.delim = (uint32_t)delimiter;
    ca.numbers = d_numbers;
    ca.count = count;
    ca.before = before;
    ca.after = after;
    ca.out_begin = d_begin;
    ca.out_end = d_end;
    ca.out_number = d_number;
    ca.out_kind = d_kind;
    ca.capacity = capacity;
    HIP_TRY(ss::launch_context_census(ca, st));
    HIP_TRY(ss::launch_context_part_prefix(ca, st));
    HIP_TRY(ss::launch_context_ranges(ca, st));
    HIP_TRY(ss::launch_context_block_prefix(ca, st));
    if (capacity != 0 && (d_number || d_kind)) {
        DeviceInfo di;
        if (int rc = device_info(pd->dev, &di)) return rc;
        HIP_TRY(ss::launch_context_fill(ca, di.cus, st));
    }
    if (capacity != 0 && (d_begin || d_end)) HIP_TRY(ss::launch_context_select(ca, st));
    HIP_TRY(hipMemcpyAsync(lease.sc.h, ca.total, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    lease.done = true;
    *lines = *lease.sc.h;
    return SS_OK;
}

// the temporary numbers of ss_find_lines_context_device, returned on every way out
struct DeviceNumbers {
    uint64_t *d = nullptr;
    ~DeviceNumbers() { if (d) (void)hipFree(d); }
};

}  // namespace
}  // namespace ssh

using namespace ssh;

extern "C" {

int ss_lines_around_device(const ss_searcher *s, const void *d_haystack, size_t len, int delimiter, const uint64_t *d_numbers,
                           uint64_t count, uint64_t before, uint64_t after, void *hip_stream, uint64_t *d_begin, uint64_t *d_end,
                           uint64_t *d_number, uint8_t *d_kind, uint64_t capacity, uint64_t *lines)
{
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    if (int rc = check_context_args(s, d_haystack, len, delimiter, lines, "ss_lines_around_device", st)) return rc;
    return lines_around(s, d_haystack, len, delimiter, d_numbers, count, before, after, st, d_begin, d_end, d_number, d_kind, capacity, lines);
}

int ss_find_lines_context_device(const ss_searcher *s, const void *d_haystack, size_t len, int delimiter, unsigned how, uint64_t before,
                                 uint64_t after, void *hip_stream, uint64_t *d_begin, uint64_t *d_end, uint64_t *d_number,
                                 uint8_t *d_kind, uint64_t capacity, uint64_t *lines, uint64_t *selected)
{
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    if (!selected) return fail(SS_ERR_ARGUMENT, "NULL argument");
    if (int rc = check_context_args(s, d_haystack, len, delimiter, lines, "ss_find_lines_context_device", st)) return rc;
    if (how & ~(SS_BOUND_WORD | SS_BOUND_LINE | SS_BOUND_NOCASE | SS_CONTEXT_INVERT))
        return fail(SS_ERR_ARGUMENT, "ss_find_lines_context_device: how = 0x%x holds bits other than SS_BOUND_WORD | SS_BOUND_LINE | "
                    "SS_BOUND_NOCASE | SS_CONTEXT_INVERT", how);
    const unsigned model = how & ~SS_CONTEXT_INVERT;
    // the model's record call with `number` only (capacity 0: its count)
    auto run = [&](uint64_t *d_out, uint64_t cap, uint64_t *n) {
        if (how & SS_CONTEXT_INVERT)
            return ss_find_lines_inverted_device(s, d_haystack, len, delimiter, model, hip_stream, nullptr, nullptr, d_out, cap, n);
        if (model & (SS_BOUND_WORD | SS_BOUND_LINE))
            return ss_find_lines_bounded_device(s, d_haystack, len, delimiter, model, hip_stream, nullptr, nullptr, d_out, cap, n);
        if (model & SS_BOUND_NOCASE)
            return ss_find_lines_nocase_device(s, d_haystack, len, delimiter, hip_stream, nullptr, nullptr, d_out, cap, n);
        return ss_find_lines_device(s, d_haystack, len, delimiter, hip_stream, nullptr, nullptr, d_out, cap, n);
    };
    uint64_t count = 0;
    if (int rc = run(nullptr, 0, &count)) return rc;
    DeviceNumbers numbers;
    if (count) {
        if (count > SIZE_MAX / sizeof(uint64_t))
            return fail(SS_ERR_NOMEM, "ss_find_lines_context_device: %llu selected lines are too many to number", (unsigned long long)count);
        const hipError_t e = hipMalloc(reinterpret_cast<void **>(&numbers.d), count * sizeof(uint64_t));
        if (e != hipSuccess) {
            (void)hipGetLastError();
            numbers.d = nullptr;
            return fail(e == hipErrorOutOfMemory ? SS_ERR_NOMEM : SS_ERR_HIP, "ss_find_lines_context_device: %llu bytes for the numbers of the selected lines: %s",
                        (unsigned long long)(count * sizeof(uint64_t)), hipGetErrorString(e));
        }
        uint64_t again = 0;
        if (int rc = run(numbers.d, count, &again)) return rc;
        if (again < count) count = again;                           // (the haystack changed under the call: stay inside what was written)
    }
    uint64_t total = 0;
    if (int rc = lines_around(s, d_haystack, len, delimiter, numbers.d, count, before, after, st, d_begin, d_end, d_number, d_kind, capacity, &total))
        return rc;
    *lines = total;
    *selected = count;
    return SS_OK;
}

}  // extern "C"
