// ss_anyof.hip - the lines that match any of several needles (include/sliceslice_hip_anyof.h): ss_union_numbers_device,
// ss_count_lines_anyof_device and ss_find_lines_anyof_device.  NOT in the other libraries: libsliceslice_hip_anyof.so holds the
// context library's objects plus this file.
//
// ss_union_numbers_device is the primitive: one workgroup per segment of SS_ANYOF_SEGMENT_LINES numbers marks the lists' entries
// in a bitmap in LDS and counts them (anyof_count_kernel), a prefix over the counts ranks the segments, and - when the numbers
// are wanted - anyof_emit_kernel builds the bitmaps of the segments below the capacity again and writes them out.  The two line
// calls count every needle's lines with its model, let the model's record call write their numbers into temporary device memory,
// one list per needle, take the number of lines from the context primitive's delimiter census and hand the union (or its
// complement) to that primitive; they call the models through their public entry points, so every refusal is theirs.
#include "ss_internal.hpp"

#include "../../include/sliceslice_hip_anyof.h"
#include "anyof_kernels.hpp"
#include "matches_host.hpp"
#include "matches_scratch.hpp"

namespace ss {

hipError_t launch_anyof_count(const AnyArgs &aa, hipStream_t st)
{
    hipLaunchKernelGGL(anyof_count_kernel, dim3((unsigned)aa.segs), dim3(kBlock), 0, st, aa);
    return hipGetLastError();
}

hipError_t launch_anyof_prefix(const AnyArgs &aa, hipStream_t st)
{
    hipLaunchKernelGGL(prefix_kernel<uint64_t>, dim3(1), dim3(kPrefixThreads), 0, st, (const uint64_t *)aa.cnt, aa.segs, aa.pre, aa.total);
    return hipGetLastError();
}

hipError_t launch_anyof_emit(const AnyArgs &aa, hipStream_t st)
{
    hipLaunchKernelGGL(anyof_emit_kernel, dim3((unsigned)aa.segs), dim3(kBlock), 0, st, aa);
    return hipGetLastError();
}

}  // namespace ss

namespace ssh {
namespace {

constexpr uint64_t kGridMax = 0x7fffffffull;
constexpr unsigned kHowBits = SS_BOUND_WORD | SS_BOUND_LINE | SS_BOUND_NOCASE | SS_CONTEXT_INVERT;

// [total: 32 bytes][cnt x segs][pre x segs][off x (lists + 1)]
int union_numbers(const ss_searcher *s, const uint64_t *d_numbers, const uint64_t *offsets, uint32_t lists, uint64_t limit, int complement,
                  hipStream_t st, uint64_t *d_out, uint64_t capacity, uint64_t *total)
{
    if (lists > SS_ANYOF_MAX_NEEDLES)
        return fail(SS_ERR_ARGUMENT, "ss_union_numbers_device: %u lists; a call takes %u", lists, (unsigned)SS_ANYOF_MAX_NEEDLES);
    if (lists != 0 && !offsets) return fail(SS_ERR_ARGUMENT, "ss_union_numbers_device: offsets is NULL and lists is %u", lists);
    for (uint32_t k = 0; k < lists; ++k)
        if (offsets[k] > offsets[k + 1])
            return fail(SS_ERR_ARGUMENT, "ss_union_numbers_device: offsets[%u] = %llu is above offsets[%u] = %llu", k,
                        (unsigned long long)offsets[k], k + 1, (unsigned long long)offsets[k + 1]);
    if (lists != 0 && offsets[lists] > offsets[0] && !d_numbers)
        return fail(SS_ERR_ARGUMENT, "ss_union_numbers_device: d_numbers is NULL and the lists hold %llu numbers",
                    (unsigned long long)(offsets[lists] - offsets[0]));
    ss::AnyArgs aa = {};
    aa.segs = ss::AnySeg::segments(limit);
    if (aa.segs > kGridMax)
        return fail(SS_ERR_ARGUMENT, "a limit of %llu needs %llu segments of %u numbers; a grid holds 2^31 - 1", (unsigned long long)limit,
                    (unsigned long long)aa.segs, (unsigned)SS_ANYOF_SEGMENT_LINES);
    if (stream_is_capturing(st))
        return fail(SS_ERR_ARGUMENT, "ss_union_numbers_device waits for its stream and cannot be captured into a hipGraph");
    *total = 0;
    if (limit == 0 || (!complement && (lists == 0 || offsets[lists] == offsets[0]))) return SS_OK;
    PerDevice *pd = nullptr;
    if (int rc = get_per_device(s, &pd)) return rc;
    ScratchLease lease;
    if (int rc = take_scratch(pd->dev, 32 + (2 * aa.segs + lists + 1) * sizeof(uint64_t), &lease.sc, st)) return rc;
    uint64_t *w = reinterpret_cast<uint64_t *>(lease.sc.d);
    aa.total = w;
    aa.cnt = w + 4;
    aa.pre = aa.cnt + aa.segs;
    uint64_t *d_off = aa.pre + aa.segs;
    aa.numbers = d_numbers;
    aa.off = d_off;
    aa.lists = lists;
    aa.complement = complement ? 1 : 0;
    aa.limit = limit;
    aa.out = d_out;
    aa.capacity = d_out ? capacity : 0;
    if (lists) HIP_TRY(hipMemcpyAsync(d_off, offsets, ((size_t)lists + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, st));
    HIP_TRY(ss::launch_anyof_count(aa, st));
    HIP_TRY(ss::launch_anyof_prefix(aa, st));
    if (aa.capacity != 0) HIP_TRY(ss::launch_anyof_emit(aa, st));
    HIP_TRY(hipMemcpyAsync(lease.sc.h, aa.total, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    lease.done = true;
    *total = *lease.sc.h;
    return SS_OK;
}

// temporary device memory of a line call, returned on every way out
struct DeviceWords {
    uint64_t *d = nullptr;
    ~DeviceWords() { if (d) (void)hipFree(d); }
    int take(uint64_t words, const char *name, const char *what)
    {
        if (words > SIZE_MAX / sizeof(uint64_t)) return fail(SS_ERR_NOMEM, "%s: %llu %s are too many to hold", name, (unsigned long long)words, what);
        const hipError_t e = hipMalloc(reinterpret_cast<void **>(&d), words * sizeof(uint64_t));
        if (e == hipSuccess) return SS_OK;
        (void)hipGetLastError();
        d = nullptr;
        return fail(e == hipErrorOutOfMemory ? SS_ERR_NOMEM : SS_ERR_HIP, "%s: %llu bytes for the %s: %s", name,
                    (unsigned long long)(words * sizeof(uint64_t)), what, hipGetErrorString(e));
    }
};

// Both line calls.  `find`: records and context are wanted (else the five output arguments are unused).
int lines_anyof(const char *name, bool find, const ss_searcher *const *searchers, uint32_t needles, const void *d_haystack, size_t len,
                int delimiter, unsigned how, uint64_t before, uint64_t after, void *hip_stream, uint64_t *d_begin, uint64_t *d_end,
                uint64_t *d_number, uint8_t *d_kind, uint64_t capacity, uint64_t *lines, uint64_t *selected)
{
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    if (!searchers || !lines || !selected) return fail(SS_ERR_ARGUMENT, "NULL argument");
    if (needles == 0) return fail(SS_ERR_ARGUMENT, "%s: no needles", name);
    if (needles > SS_ANYOF_MAX_NEEDLES) return fail(SS_ERR_ARGUMENT, "%s: %u needles; a call takes %u", name, needles, (unsigned)SS_ANYOF_MAX_NEEDLES);
    for (uint32_t k = 0; k < needles; ++k)
        if (!searchers[k]) return fail(SS_ERR_ARGUMENT, "%s: searchers[%u] is NULL", name, k);
    if (int rc = check_common_args(searchers[0], d_haystack, len, lines)) return rc;
    if (delimiter < 0 || delimiter > 255) return fail(SS_ERR_ARGUMENT, "delimiter %d is not a byte (0 .. 255)", delimiter);
    if (stream_is_capturing(st)) return fail(SS_ERR_ARGUMENT, "%s waits for its stream and cannot be captured into a hipGraph", name);
    if (how & ~kHowBits)
        return fail(SS_ERR_ARGUMENT, "%s: how = 0x%x holds bits other than SS_BOUND_WORD | SS_BOUND_LINE | SS_BOUND_NOCASE | SS_CONTEXT_INVERT", name, how);
    const unsigned model = how & ~SS_CONTEXT_INVERT;
    const int complement = (how & SS_CONTEXT_INVERT) ? 1 : 0;
    // the NON-inverted model's record call with `number` only (capacity 0: its count)
    auto run = [&](const ss_searcher *s, uint64_t *d_out, uint64_t cap, uint64_t *n) {
        if (model & (SS_BOUND_WORD | SS_BOUND_LINE))
            return ss_find_lines_bounded_device(s, d_haystack, len, delimiter, model, hip_stream, nullptr, nullptr, d_out, cap, n);
        if (model & SS_BOUND_NOCASE)
            return ss_find_lines_nocase_device(s, d_haystack, len, delimiter, hip_stream, nullptr, nullptr, d_out, cap, n);
        return ss_find_lines_device(s, d_haystack, len, delimiter, hip_stream, nullptr, nullptr, d_out, cap, n);
    };
    // every needle's count first: a refusal of any model comes before anything is written
    std::vector<uint64_t> off((size_t)needles + 1, 1);                      // (word 0 of the buffer holds the number 1, for the census)
    uint64_t most = 0;
    for (uint32_t k = 0; k < needles; ++k) {
        uint64_t n = 0;
        if (int rc = run(searchers[k], nullptr, 0, &n)) return rc;
        if (n > UINT64_MAX / 4 - off[k]) return fail(SS_ERR_NOMEM, "%s: the selected lines are too many to number", name);
        off[k + 1] = off[k] + n;
        if (n > most) most = n;
    }
    const uint64_t sum = off[needles] - 1;
    *lines = 0;
    *selected = 0;
    if (len == 0 || (!complement && sum == 0)) return SS_OK;
    // [1][the needles' numbers: sum][the union, where it is known to fit into `sum` words]
    const bool own_union = find && !complement;
    DeviceWords numbers, inverse;
    if (int rc = numbers.take(1 + sum + (own_union ? sum : 0), name, "numbers of the selected lines")) return rc;
    static const uint64_t kOne = 1;
    HIP_TRY(hipMemcpyAsync(numbers.d, &kOne, sizeof(uint64_t), hipMemcpyHostToDevice, st));
    for (uint32_t k = 0; k < needles; ++k) {
        const uint64_t n = off[k + 1] - off[k];
        if (n == 0) continue;
        uint64_t again = 0;
        if (int rc = run(searchers[k], numbers.d + off[k], n, &again)) return rc;
        if (again < n)                                                      // (the haystack changed under the call: a 0 selects nothing)
            HIP_TRY(hipMemsetAsync(numbers.d + off[k] + again, 0, (n - again) * sizeof(uint64_t), st));
    }
    // N from the delimiter census: the lines from line 1 to the end of the view, counted only
    uint64_t N = 0;
    if (int rc = ss_lines_around_device(searchers[0], d_haystack, len, delimiter, numbers.d, 1, 0, ~0ull, hip_stream, nullptr, nullptr, nullptr,
                                        nullptr, 0, &N))
        return rc;
    uint64_t *d_union = nullptr, room = 0;
    if (own_union) {
        d_union = numbers.d + 1 + sum;
        room = sum;
    } else if (find) {
        room = N > most ? N - most : 0;                                     // the complement holds no line of the largest S_k
        if (room) {
            if (int rc = inverse.take(room, name, "numbers of the lines that match no needle")) return rc;
            d_union = inverse.d;
        }
    }
    uint64_t total = 0;
    if (int rc = union_numbers(searchers[0], numbers.d, off.data(), needles, N, complement, st, d_union, room, &total)) return rc;
    if (find) {
        uint64_t printed = 0;
        if (int rc = ss_lines_around_device(searchers[0], d_haystack, len, delimiter, d_union, total < room ? total : room, before, after,
                                            hip_stream, d_begin, d_end, d_number, d_kind, capacity, &printed))
            return rc;
        *lines = printed;
        *selected = total;
    } else {
        *lines = total;
    }
    return SS_OK;
}

}  // namespace
}  // namespace ssh

using namespace ssh;

extern "C" {

int ss_union_numbers_device(const ss_searcher *s, const uint64_t *d_numbers, const uint64_t *offsets, uint32_t lists, uint64_t limit,
                            int complement, void *hip_stream, uint64_t *d_out, uint64_t capacity, uint64_t *total)
{
    if (!s || !total) return fail(SS_ERR_ARGUMENT, "NULL argument");
    return union_numbers(s, d_numbers, offsets, lists, limit, complement, static_cast<hipStream_t>(hip_stream), d_out, capacity, total);
}

int ss_count_lines_anyof_device(const ss_searcher *const *searchers, uint32_t needles, const void *d_haystack, size_t len, int delimiter,
                                unsigned how, void *hip_stream, uint64_t *lines)
{
    uint64_t unused = 0;
    return lines_anyof("ss_count_lines_anyof_device", false, searchers, needles, d_haystack, len, delimiter, how, 0, 0, hip_stream, nullptr,
                       nullptr, nullptr, nullptr, 0, lines, &unused);
}

int ss_find_lines_anyof_device(const ss_searcher *const *searchers, uint32_t needles, const void *d_haystack, size_t len, int delimiter,
                               unsigned how, uint64_t before, uint64_t after, void *hip_stream, uint64_t *d_begin, uint64_t *d_end,
                               uint64_t *d_number, uint8_t *d_kind, uint64_t capacity, uint64_t *lines, uint64_t *selected)
{
    return lines_anyof("ss_find_lines_anyof_device", true, searchers, needles, d_haystack, len, delimiter, how, before, after, hip_stream,
                       d_begin, d_end, d_number, d_kind, capacity, lines, selected);
}

}  // extern "C"
