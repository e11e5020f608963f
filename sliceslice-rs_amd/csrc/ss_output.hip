// ss_output.hip - grep's output written on the device (include/sliceslice_hip_output.h): ss_format_lines_device,
// ss_gather_ranges_device and ss_grep_lines_device.  NOT in the other libraries: libsliceslice_hip_output.so holds the disjoint
// library's objects plus this file.
//
// The format call is four launches (output_kernels.hpp): the blocks' bytes, the prefix over the blocks, the records' starts, and the
// copy over the output's chunks.  The total comes back after the first three; a capacity below it ends the call there.  The gather
// call is the format call without flags.  The grep call is ss_find_lines_context_device through its public entry point - first its
// count, then its four arrays into temporary device memory - and the format call on those records.
#include "ss_internal.hpp"

#include "../../include/sliceslice_hip_output.h"
#include "matches_host.hpp"
#include "matches_scratch.hpp"
#include "output_kernels.hpp"

namespace ss {

hipError_t launch_output_sizes(const OutputArgs &a, hipStream_t st)
{
    hipLaunchKernelGGL(output_sizes_kernel, dim3((unsigned)a.blocks), dim3(kOutputThreads), 0, st, a);
    if (hipError_t e = hipGetLastError()) return e;
    hipLaunchKernelGGL((prefix_kernel<uint64_t>), dim3(1), dim3(kPrefixThreads), 0, st, (const uint64_t *)a.sum, a.blocks, a.rank, a.total);
    return hipGetLastError();
}

hipError_t launch_output_starts(const OutputArgs &a, hipStream_t st)
{
    hipLaunchKernelGGL(output_starts_kernel, dim3((unsigned)a.blocks), dim3(kOutputThreads), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_output_copy(const OutputArgs &a, hipStream_t st)
{
    hipLaunchKernelGGL(output_copy_kernel, dim3((unsigned)a.chunks), dim3(kOutputCopyThreads), 0, st, a);
    return hipGetLastError();
}

}  // namespace ss

namespace ssh {
namespace {

constexpr uint64_t kGridMax = 0x7fffffffull;
constexpr uint64_t kOutputCountMax = 1ull << 48;

// temporary device memory of a call, returned on every way out
struct DeviceBytes {
    uint8_t *d = nullptr;
    ~DeviceBytes() { if (d) (void)hipFree(d); }
    int take(uint64_t bytes, const char *name, const char *what)
    {
        if (bytes > SIZE_MAX) return fail(SS_ERR_NOMEM, "%s: %llu bytes for the %s are too many to hold", name, (unsigned long long)bytes, what);
        const hipError_t e = hipMalloc(reinterpret_cast<void **>(&d), (size_t)bytes);
        if (e == hipSuccess) return SS_OK;
        (void)hipGetLastError();
        d = nullptr;
        return fail(e == hipErrorOutOfMemory ? SS_ERR_NOMEM : SS_ERR_HIP, "%s: %llu bytes for the %s: %s", name, (unsigned long long)bytes, what,
                    hipGetErrorString(e));
    }
};

// what the format and the gather call refuse
int check_output_args(const char *name, const ss_searcher *s, const void *d_haystack, size_t len, const uint64_t *d_begin, const uint64_t *d_end,
                      const uint64_t *d_number, uint64_t count, int terminator, unsigned flags, hipStream_t st, const void *d_out,
                      uint64_t out_capacity, const uint64_t *out_len)
{
    if (int rc = check_common_args(s, d_haystack, len, out_len)) return rc;
    if (flags & ~(SS_OUTPUT_NUMBER | SS_OUTPUT_SEPARATOR))
        return fail(SS_ERR_ARGUMENT, "%s: flags = 0x%x holds bits other than SS_OUTPUT_NUMBER | SS_OUTPUT_SEPARATOR", name, flags);
    if (terminator < -1 || terminator > 255) return fail(SS_ERR_ARGUMENT, "%s: the terminator is one byte, 0..255, or -1 for none; got %d", name, terminator);
    if (count != 0 && flags != 0 && !d_number)
        return fail(SS_ERR_ARGUMENT, "%s: d_number is NULL and flags = 0x%x asks for line numbers or separators", name, flags);
    if (count != 0 && (!d_begin || !d_end)) return fail(SS_ERR_ARGUMENT, "%s: d_begin or d_end is NULL and count is %llu", name, (unsigned long long)count);
    if (count >= kOutputCountMax) return fail(SS_ERR_ARGUMENT, "%s: %llu records; a call takes fewer than 2^48", name, (unsigned long long)count);
    const uintptr_t h0 = reinterpret_cast<uintptr_t>(d_haystack), o0 = reinterpret_cast<uintptr_t>(d_out);
    if (d_out && len != 0 && out_capacity != 0 && o0 < h0 + len && h0 < o0 + out_capacity)
        return fail(SS_ERR_ARGUMENT, "%s: d_out[0, %llu) intersects the haystack; the output is not written in place", name,
                    (unsigned long long)out_capacity);
    if (stream_is_capturing(st)) return fail(SS_ERR_ARGUMENT, "%s waits for its stream and cannot be captured into a hipGraph", name);
    return SS_OK;
}

// The format call behind its argument checks.  Scratch from the free list: [total: 32 bytes][sum x blocks][rank x blocks].
int format_lines(const char *name, const ss_searcher *s, const void *d_haystack, size_t len, const uint64_t *d_begin, const uint64_t *d_end,
                 const uint64_t *d_number, const uint8_t *d_kind, uint64_t count, int terminator, unsigned flags, hipStream_t st, void *d_out,
                 uint64_t out_capacity, uint64_t *d_starts, uint64_t *out_len)
{
    *out_len = 0;
    if (count == 0) {
        if (d_starts) {
            HIP_TRY(hipMemsetAsync(d_starts, 0, sizeof(uint64_t), st));
            HIP_TRY(hipStreamSynchronize(st));
        }
        return SS_OK;
    }
    ss::OutputArgs a = {};
    a.hay = static_cast<const uint8_t *>(d_haystack);
    a.len = len;
    a.begin = d_begin;
    a.end = d_end;
    a.number = flags ? d_number : nullptr;
    a.kind = d_kind;
    a.count = count;
    a.blocks = (count + SS_OUTPUT_BLOCK - 1) / SS_OUTPUT_BLOCK;
    a.terminator = terminator;
    a.flags = flags;
    if (a.blocks > kGridMax)
        return fail(SS_ERR_ARGUMENT, "%s: %llu records need %llu blocks of %u; a grid holds 2^31 - 1", name, (unsigned long long)count,
                    (unsigned long long)a.blocks, (unsigned)SS_OUTPUT_BLOCK);
    PerDevice *pd = nullptr;
    if (int rc = get_per_device(s, &pd)) return rc;
    ScratchLease lease;
    if (int rc = take_scratch(pd->dev, 32 + a.blocks * 16, &lease.sc, st)) return rc;
    uint64_t *w = reinterpret_cast<uint64_t *>(lease.sc.d);
    a.total = w;
    a.sum = w + 4;
    a.rank = a.sum + a.blocks;
    a.starts = d_starts;
    HIP_TRY(ss::launch_output_sizes(a, st));
    if (a.starts) HIP_TRY(ss::launch_output_starts(a, st));
    HIP_TRY(hipMemcpyAsync(lease.sc.h, a.total, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    const uint64_t total = *lease.sc.h;
    *out_len = total;
    if (out_capacity < total || total == 0) {
        lease.done = true;
        return SS_OK;
    }
    if (!d_out) {
        lease.done = true;
        return fail(SS_ERR_ARGUMENT, "%s: d_out is NULL and the output holds %llu bytes", name, (unsigned long long)total);
    }
    DeviceBytes starts;
    if (!a.starts) {
        if (int rc = starts.take((count + 1) * sizeof(uint64_t), name, "records' starts")) {
            lease.done = true;
            return rc;
        }
        a.starts = reinterpret_cast<uint64_t *>(starts.d);
        HIP_TRY(ss::launch_output_starts(a, st));
    }
    const uint64_t mis = (uint64_t)(reinterpret_cast<uintptr_t>(d_out) & 15);
    a.out_base = static_cast<uint8_t *>(d_out) - mis;
    a.out_lo = mis;
    a.out_hi = mis + total;
    a.chunks = (a.out_hi + SS_OUTPUT_CHUNK - 1) / SS_OUTPUT_CHUNK;
    if (a.chunks > kGridMax)
        return fail(SS_ERR_ARGUMENT, "%s: an output of %llu bytes needs %llu chunks of %u bytes; a grid holds 2^31 - 1", name,
                    (unsigned long long)total, (unsigned long long)a.chunks, (unsigned)SS_OUTPUT_CHUNK);
    HIP_TRY(ss::launch_output_copy(a, st));
    HIP_TRY(hipStreamSynchronize(st));
    lease.done = true;
    return SS_OK;
}

}  // namespace
}  // namespace ssh

using namespace ssh;

extern "C" {

int ss_format_lines_device(const ss_searcher *s, const void *d_haystack, size_t len, const uint64_t *d_begin, const uint64_t *d_end,
                           const uint64_t *d_number, const uint8_t *d_kind, uint64_t count, int terminator, unsigned flags, void *hip_stream,
                           void *d_out, uint64_t out_capacity, uint64_t *d_starts, uint64_t *out_len)
{
    const char *name = "ss_format_lines_device";
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    if (int rc = check_output_args(name, s, d_haystack, len, d_begin, d_end, d_number, count, terminator, flags, st, d_out, out_capacity, out_len))
        return rc;
    return format_lines(name, s, d_haystack, len, d_begin, d_end, d_number, d_kind, count, terminator, flags, st, d_out, out_capacity, d_starts,
                        out_len);
}

int ss_gather_ranges_device(const ss_searcher *s, const void *d_haystack, size_t len, const uint64_t *d_begin, const uint64_t *d_end,
                            uint64_t count, int terminator, void *hip_stream, void *d_out, uint64_t out_capacity, uint64_t *d_starts,
                            uint64_t *out_len)
{
    const char *name = "ss_gather_ranges_device";
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    if (int rc = check_output_args(name, s, d_haystack, len, d_begin, d_end, nullptr, count, terminator, 0, st, d_out, out_capacity, out_len))
        return rc;
    return format_lines(name, s, d_haystack, len, d_begin, d_end, nullptr, nullptr, count, terminator, 0, st, d_out, out_capacity, d_starts,
                        out_len);
}

int ss_grep_lines_device(const ss_searcher *s, const void *d_haystack, size_t len, int delimiter, unsigned how, uint64_t before, uint64_t after,
                         unsigned flags, void *hip_stream, void *d_out, uint64_t out_capacity, uint64_t *out_len, uint64_t *lines,
                         uint64_t *selected)
{
    const char *name = "ss_grep_lines_device";
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    if (!out_len || !lines || !selected) return fail(SS_ERR_ARGUMENT, "NULL argument");
    if (flags & ~(SS_OUTPUT_NUMBER | SS_OUTPUT_SEPARATOR))
        return fail(SS_ERR_ARGUMENT, "%s: flags = 0x%x holds bits other than SS_OUTPUT_NUMBER | SS_OUTPUT_SEPARATOR", name, flags);
    const uintptr_t h0 = reinterpret_cast<uintptr_t>(d_haystack), o0 = reinterpret_cast<uintptr_t>(d_out);
    if (d_out && d_haystack && len != 0 && out_capacity != 0 && o0 < h0 + len && h0 < o0 + out_capacity)
        return fail(SS_ERR_ARGUMENT, "%s: d_out[0, %llu) intersects the haystack; the output is not written in place", name,
                    (unsigned long long)out_capacity);
    // the records: the count, then all four arrays into memory of the call's own
    uint64_t total = 0, sel = 0;
    if (int rc = ss_find_lines_context_device(s, d_haystack, len, delimiter, how, before, after, hip_stream, nullptr, nullptr, nullptr, nullptr, 0,
                                              &total, &sel))
        return rc;
    *out_len = 0;
    *lines = total;
    *selected = sel;
    if (total == 0) return SS_OK;
    if (total >= kOutputCountMax) return fail(SS_ERR_ARGUMENT, "%s: %llu lines; a call takes fewer than 2^48", name, (unsigned long long)total);
    DeviceBytes rec;
    if (int rc = rec.take(total * 25, name, "records of the printed lines")) return rc;
    uint64_t *d_begin = reinterpret_cast<uint64_t *>(rec.d), *d_end = d_begin + total, *d_number = d_end + total;
    uint8_t *d_kind = reinterpret_cast<uint8_t *>(d_number + total);
    uint64_t again = 0, sel2 = 0;
    if (int rc = ss_find_lines_context_device(s, d_haystack, len, delimiter, how, before, after, hip_stream, d_begin, d_end, d_number, d_kind, total,
                                              &again, &sel2))
        return rc;
    if (again != total)
        return fail(SS_ERR_ARGUMENT, "%s: the haystack changed under the call (%llu lines, then %llu)", name, (unsigned long long)total,
                    (unsigned long long)again);
    return format_lines(name, s, d_haystack, len, d_begin, d_end, d_number, d_kind, total, delimiter, flags, st, d_out, out_capacity, nullptr, out_len);
}

}  // extern "C"
