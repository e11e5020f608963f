// ss_classes.hip - fixed-length patterns of byte classes, searched in ONE pass over the haystack
// (include/sliceslice_hip_classes.h has THE RULE and the pattern language): ss_classes_new / _free / _info, ss_classes_parse,
// ss_classes_cover, ss_count_classes_device / _async, ss_find_all_classes_device, ss_count_lines_classes_device and
// ss_find_lines_classes_device.  NOT in the other libraries: libsliceslice_hip_classes.so holds the masked library's objects plus
// this file.
//
// A pattern is its plan (classes_host.hpp: covers, distinct inexact sets, check list, filter positions) and ONE device allocation:
// the covers' (value, mask) dword pairs, the bitmaps, the check list.  The calls are ss_masked.hip's, launch for launch, with the
// class kernels in place of the masked ones.
#include "ss_internal.hpp"

#include "../../include/sliceslice_hip_classes.h"
#include "classes_host.hpp"
#include "classes_kernels.hpp"
#include "matches_scratch.hpp"

#include <new>

struct ss_classes {
    ssh::classes::Plan plan;
    std::vector<uint64_t> sets;             // 4 words per position
    uint32_t n = 0, a = 0, d = 0;
    uint32_t *d_tab = nullptr;              // [cover pairs, 2 * ceil(n / 4)][bitmaps, 8 per distinct set][check list]
    int dev = -1;
};

namespace ss {

hipError_t launch_classes_all(const ClassArgs &a, int mode, hipStream_t st)
{
    const dim3 grid((unsigned)((a.m.ntiles + kSetTiles - 1) / kSetTiles)), block(kBlock);
    if (mode == kMaskedCount) hipLaunchKernelGGL((classes_all_kernel<kMaskedCount>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((classes_all_kernel<kMaskedEmit>), grid, block, 0, st, a);
    return hipGetLastError();
}

hipError_t launch_classes_lines(const ClassArgs &a, int mode, hipStream_t st)
{
    const dim3 grid((unsigned)((a.m.ntiles + kSetTiles - 1) / kSetTiles)), block(kBlock);
    if (mode == kMaskedSum) hipLaunchKernelGGL((classes_lines_kernel<kMaskedSum>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((classes_lines_kernel<kMaskedLineEmit>), grid, block, 0, st, a);
    return hipGetLastError();
}

}  // namespace ss

namespace ssh {
namespace {

// What every scan refuses, and the argument block of the view.  `waits`: the call waits for its stream.
int classes_args(const char *name, const ss_classes *p, const void *d_haystack, size_t len, bool waits, hipStream_t st, ss::ClassArgs *ca)
{
    if (!p) return fail(SS_ERR_ARGUMENT, "%s: the pattern is NULL", name);
    if (len && !d_haystack) return fail(SS_ERR_ARGUMENT, "%s: haystack is NULL", name);
    if (waits && stream_is_capturing(st)) return fail(SS_ERR_ARGUMENT, "%s waits for its stream and cannot be captured into a hipGraph", name);
    int dev = -1;
    HIP_TRY(hipGetDevice(&dev));
    if (dev != p->dev) return fail(SS_ERR_ARGUMENT, "%s: the pattern was made on device %d, the current device is %d", name, p->dev, dev);
    const uint8_t *hay = static_cast<const uint8_t *>(d_haystack);
    *ca = ss::ClassArgs{};
    ss::MaskedArgs *a = &ca->m;
    a->mis = (uint64_t)(reinterpret_cast<uintptr_t>(hay) & 15);
    a->base = hay - a->mis;
    a->hay = hay;
    a->len = len;
    a->nchunks = (a->mis + len + 15) / 16;
    a->ntiles = (a->nchunks + ss::kSetTileChunks - 1) / ss::kSetTileChunks;
    a->tab = p->d_tab;
    a->n = p->n;
    a->nw = (p->n + 3) / 4;
    a->a = p->a;
    a->d = p->d;
    a->v0x4 = p->plan.value[p->a] * 0x01010101u;
    a->m0x4 = p->plan.mask[p->a] * 0x01010101u;
    a->v1x4 = p->d ? p->plan.value[p->a + p->d] * 0x01010101u : 0u;
    a->m1x4 = p->d ? p->plan.mask[p->a + p->d] * 0x01010101u : 0u;
    ca->ctab = p->d_tab + 2 * a->nw;
    ca->nbits = (uint32_t)(p->plan.bitmaps.size() * 2);
    ca->nchecks = (uint32_t)p->plan.checks.size();
    if ((a->ntiles + ss::kSetTiles - 1) / ss::kSetTiles > 0x7fffffffull)
        return fail(SS_ERR_ARGUMENT, "%s: a haystack of %zu bytes needs more than 2^31 - 1 workgroups", name, len);
    return SS_OK;
}

bool accepts_byte(const ss_classes *p, int byte)
{
    for (uint32_t i = 0; i < p->n; ++i)
        if (classes::set_has(&p->sets[4 * (size_t)i], (unsigned)byte)) return true;
    return false;
}

// Both line calls.  `find`: records are wanted (else the four output arguments are unused).
int lines_classes(const char *name, bool find, const ss_classes *p, const void *d_haystack, size_t len, int delimiter, void *hip_stream,
                  uint64_t *d_begin, uint64_t *d_end, uint64_t *d_number, uint64_t capacity, uint64_t *lines)
{
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    if (!lines) return fail(SS_ERR_ARGUMENT, "%s: lines is NULL", name);
    if (delimiter < 0 || delimiter > 255) return fail(SS_ERR_ARGUMENT, "delimiter %d is not a byte (0 .. 255)", delimiter);
    ss::ClassArgs ca;
    if (int rc = classes_args(name, p, d_haystack, len, true, st, &ca)) return rc;
    if (len < p->n) {
        *lines = 0;
        return SS_OK;
    }
    ss::MaskedArgs &a = ca.m;
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
    a.accepts = accepts_byte(p, delimiter) ? 1u : 0u;
    HIP_TRY(ss::launch_classes_lines(ca, ss::kMaskedSum, st));
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
        HIP_TRY(ss::launch_classes_lines(ca, ss::kMaskedLineEmit, st));
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

int ss_classes_parse(const char *text, int ignore_case, uint64_t *sets, size_t capacity, size_t *n)
{
    if (!text || !n) return fail(SS_ERR_ARGUMENT, "NULL argument");
    classes::ParseError err = {0, nullptr};
    try {
        if (!classes::parse_classes(text, ignore_case != 0, sets, capacity, n, &err))
            return fail(SS_ERR_ARGUMENT, "ss_classes_parse: column %zu: %s", err.column, err.what);
    } catch (const std::bad_alloc &) {
        return fail(SS_ERR_NOMEM, "ss_classes_parse: out of memory");
    }
    return SS_OK;
}

int ss_classes_cover(const uint64_t *sets, size_t n, uint8_t *value, uint8_t *mask)
{
    if (n && !sets) return fail(SS_ERR_ARGUMENT, "NULL argument");
    for (size_t i = 0; i < n; ++i)
        if (classes::set_size(sets + 4 * i) == 0) return fail(SS_ERR_ARGUMENT, "ss_classes_cover: the set of position %zu is empty", i);
    for (size_t i = 0; i < n; ++i) {
        uint8_t v, m;
        classes::class_cover(sets + 4 * i, &v, &m);
        if (value) value[i] = v;
        if (mask) mask[i] = m;
    }
    return SS_OK;
}

int ss_classes_new(const uint64_t *sets, size_t n, ss_classes **pattern)
{
    if (!pattern) return fail(SS_ERR_ARGUMENT, "NULL argument");
    if (n == 0 || n > SS_CLASSES_MAX_LEN)
        return fail(SS_ERR_ARGUMENT, "ss_classes_new: a pattern holds 1 .. %d positions (SS_CLASSES_MAX_LEN), not %zu", SS_CLASSES_MAX_LEN, n);
    if (!sets) return fail(SS_ERR_ARGUMENT, "NULL argument");
    ss_classes *p = new (std::nothrow) ss_classes;
    if (!p) return fail(SS_ERR_NOMEM, "ss_classes_new: out of memory");
    struct Guard {
        ss_classes *p;
        ~Guard() { if (p) ss_classes_free(p); }
    } guard{p};
    const size_t nw = (n + 3) / 4;
    std::vector<uint32_t> tab;
    try {
        const ByteCost cost(nullptr);
        size_t where = 0;
        switch (classes::make_class_plan(sets, n, cost.cost, &p->plan, &where)) {
        case classes::kPlanOk:
            break;
        case classes::kPlanEmptySet:
            return fail(SS_ERR_ARGUMENT, "ss_classes_new: the set of position %zu is empty", where);
        case classes::kPlanTooManyInexact:
            return fail(SS_ERR_ARGUMENT, "ss_classes_new: more than %d positions whose set is not exactly its cover (SS_CLASSES_MAX_INEXACT)",
                        SS_CLASSES_MAX_INEXACT);
        case classes::kPlanTooManyDistinct:
            return fail(SS_ERR_ARGUMENT, "ss_classes_new: more than %d distinct sets that are not exactly their cover (SS_CLASSES_MAX_DISTINCT)",
                        SS_CLASSES_MAX_DISTINCT);
        }
        p->sets.assign(sets, sets + 4 * n);
        const classes::Plan &plan = p->plan;
        tab.assign(2 * nw, 0u);
        for (size_t i = 0; i < n; ++i) {
            tab[2 * (i / 4)] |= (uint32_t)plan.value[i] << (8 * (i % 4));
            tab[2 * (i / 4) + 1] |= (uint32_t)plan.mask[i] << (8 * (i % 4));
        }
        for (uint64_t w : plan.bitmaps) {
            tab.push_back((uint32_t)w);
            tab.push_back((uint32_t)(w >> 32));
        }
        for (uint32_t e : plan.checks) tab.push_back((e & 0xFFFFu) | (8u * (e >> 16)) << 16);
    } catch (const std::bad_alloc &) {
        return fail(SS_ERR_NOMEM, "ss_classes_new: out of memory");
    }
    p->n = (uint32_t)n;
    size_t a = 0, d = 0;
    if (int rc = classes::choose_class_filter(p->plan, &a, &d)) return rc;
    p->a = (uint32_t)a;
    p->d = (uint32_t)d;
    HIP_TRY(hipGetDevice(&p->dev));
    const hipError_t e = hipMalloc(reinterpret_cast<void **>(&p->d_tab), tab.size() * 4);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        p->d_tab = nullptr;
        return fail(e == hipErrorOutOfMemory ? SS_ERR_NOMEM : SS_ERR_HIP, "ss_classes_new: %zu bytes for the tables: %s", tab.size() * 4, hipGetErrorString(e));
    }
    HIP_TRY(hipMemcpy(p->d_tab, tab.data(), tab.size() * 4, hipMemcpyHostToDevice));
    guard.p = nullptr;
    *pattern = p;
    return SS_OK;
}

void ss_classes_free(ss_classes *p)
{
    if (!p) return;
    if (p->d_tab) (void)hipFree(p->d_tab);
    delete p;
}

int ss_classes_info(const ss_classes *p, int delimiter, ss_classes_stats *stats)
{
    if (!p || !stats) return fail(SS_ERR_ARGUMENT, "NULL argument");
    if (delimiter > 255) return fail(SS_ERR_ARGUMENT, "delimiter %d is not a byte (0 .. 255)", delimiter);
    const ss_classes_stats s = {p->n, p->a, p->d, p->plan.single, p->plan.masked, p->plan.inexact, p->plan.bitmaps.size() / 4,
                                delimiter >= 0 && accepts_byte(p, delimiter) ? 1u : 0u};
    *stats = s;
    return SS_OK;
}

int ss_count_classes_device_async(const ss_classes *p, const void *d_haystack, size_t len, void *hip_stream, uint64_t *d_count)
{
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    if (!d_count) return fail(SS_ERR_ARGUMENT, "ss_count_classes_device_async: d_count is NULL");
    ss::ClassArgs ca;
    if (int rc = classes_args("ss_count_classes_device_async", p, d_haystack, len, false, st, &ca)) return rc;
    HIP_TRY(hipMemsetAsync(d_count, 0, sizeof(uint64_t), st));
    if (len < p->n) return SS_OK;
    ca.m.total = d_count;
    HIP_TRY(ss::launch_classes_all(ca, ss::kMaskedCount, st));
    return SS_OK;
}

int ss_count_classes_device(const ss_classes *p, const void *d_haystack, size_t len, void *hip_stream, uint64_t *count)
{
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    if (!count) return fail(SS_ERR_ARGUMENT, "ss_count_classes_device: count is NULL");
    ss::ClassArgs ca;
    if (int rc = classes_args("ss_count_classes_device", p, d_haystack, len, true, st, &ca)) return rc;
    if (len < p->n) {
        *count = 0;
        return SS_OK;
    }
    ScratchLease lease;
    if (int rc = take_scratch(p->dev, sizeof(uint64_t), &lease.sc, st)) return rc;
    ca.m.total = reinterpret_cast<uint64_t *>(lease.sc.d);
    HIP_TRY(hipMemsetAsync(ca.m.total, 0, sizeof(uint64_t), st));
    HIP_TRY(ss::launch_classes_all(ca, ss::kMaskedCount, st));
    HIP_TRY(hipMemcpyAsync(lease.sc.h, ca.m.total, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    lease.done = true;
    *count = *lease.sc.h;
    return SS_OK;
}

int ss_find_all_classes_device(const ss_classes *p, const void *d_haystack, size_t len, void *hip_stream, uint64_t *d_offsets, uint64_t capacity,
                               uint64_t *total)
{
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    if (!total) return fail(SS_ERR_ARGUMENT, "ss_find_all_classes_device: total is NULL");
    if (capacity && !d_offsets) return fail(SS_ERR_ARGUMENT, "ss_find_all_classes_device: offsets are NULL with a capacity of %llu", (unsigned long long)capacity);
    ss::ClassArgs ca;
    if (int rc = classes_args("ss_find_all_classes_device", p, d_haystack, len, true, st, &ca)) return rc;
    if (len < p->n) {
        *total = 0;
        return SS_OK;
    }
    ss::MaskedArgs &a = ca.m;
    const uint64_t parts = (a.ntiles + ss::kSetTiles - 1) / ss::kSetTiles;
    // [total u64][rank u64 x parts][occurrences u64 x parts]
    ScratchLease lease;
    if (int rc = take_scratch(p->dev, 8 + parts * 16, &lease.sc, st)) return rc;
    uint64_t *d_total = reinterpret_cast<uint64_t *>(lease.sc.d);
    uint64_t *d_rank = d_total + 1;
    a.wg = d_rank + parts;
    HIP_TRY(ss::launch_classes_all(ca, ss::kMaskedCount, st));
    HIP_TRY(ss::launch_set_prefix(a.wg, parts, d_rank, d_total, st));
    if (capacity != 0) {
        a.wg_rank = d_rank;
        a.offsets = d_offsets;
        a.capacity = capacity;
        HIP_TRY(ss::launch_classes_all(ca, ss::kMaskedEmit, st));
    }
    HIP_TRY(hipMemcpyAsync(lease.sc.h, d_total, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    lease.done = true;
    *total = *lease.sc.h;
    return SS_OK;
}

int ss_count_lines_classes_device(const ss_classes *p, const void *d_haystack, size_t len, int delimiter, void *hip_stream, uint64_t *lines)
{
    return lines_classes("ss_count_lines_classes_device", false, p, d_haystack, len, delimiter, hip_stream, nullptr, nullptr, nullptr, 0, lines);
}

int ss_find_lines_classes_device(const ss_classes *p, const void *d_haystack, size_t len, int delimiter, void *hip_stream, uint64_t *d_begin,
                                 uint64_t *d_end, uint64_t *d_number, uint64_t capacity, uint64_t *lines)
{
    return lines_classes("ss_find_lines_classes_device", true, p, d_haystack, len, delimiter, hip_stream, d_begin, d_end, d_number, capacity,
                         lines);
}

}  // extern "C"
