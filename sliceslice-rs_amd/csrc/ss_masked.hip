// ss_masked.hip - byte patterns with wildcards and per-byte masks, searched in ONE pass over the haystack
// (include/sliceslice_hip_masked.h has THE RULE): ss_masked_new / _free / _info, ss_masked_parse_hex, ss_masked_choose_filter,
// ss_count_masked_device / _async, ss_find_all_masked_device, ss_count_lines_masked_device and ss_find_lines_masked_device.
// NOT in the other libraries: libsliceslice_hip_masked.so holds the leftmost library's objects plus this file.
//
// A pattern is its (value, mask) dword pairs in ONE device allocation and the two filter positions chosen at construction.  A call
// cuts the view into parts of kSetPartBytes from the 16-byte aligned address at or below it, one workgroup each, as
// ss_setmatches.hip and ss_needleset.hip do:
//   count   the result is zeroed on the stream, then masked_all_kernel<kMaskedCount> adds into it.  The async form needs nothing
//           else and can be captured; the waiting form keeps the total in call-owned scratch and reads it back.
//   find    the count pass with one word per workgroup, their exclusive prefix (prefix_kernel.hpp) and
//           masked_all_kernel<kMaskedEmit> over the workgroups that hold one of the first `capacity` occurrences.
//   lines   masked_lines_kernel<kMaskedSum> leaves a LineSum per part; lines_chunk_kernel and lines_combine_kernel as ss_lines.hip
//           launches them; for records the states are spread back over the parts and masked_lines_kernel<kMaskedLineEmit> writes.
// A pattern longer than the view has no occurrence and matches no line: those calls answer without a launch.
#include "ss_internal.hpp"

#include "../../include/sliceslice_hip_masked.h"
#include "masked_kernels.hpp"
#include "matches_scratch.hpp"

#include <new>

struct ss_masked {
    std::vector<uint8_t> value, mask;       // value & mask, mask
    uint32_t n = 0, a = 0, d = 0;
    uint32_t *d_tab = nullptr;              // (value, mask) dword pairs
    int dev = -1;
};

namespace ss {

hipError_t launch_masked_all(const MaskedArgs &a, int mode, hipStream_t st)
{
    const dim3 grid((unsigned)((a.ntiles + kSetTiles - 1) / kSetTiles)), block(kBlock);
    if (mode == kMaskedCount) hipLaunchKernelGGL((masked_all_kernel<kMaskedCount>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((masked_all_kernel<kMaskedEmit>), grid, block, 0, st, a);
    return hipGetLastError();
}

hipError_t launch_masked_lines(const MaskedArgs &a, int mode, hipStream_t st)
{
    const dim3 grid((unsigned)((a.ntiles + kSetTiles - 1) / kSetTiles)), block(kBlock);
    if (mode == kMaskedSum) hipLaunchKernelGGL((masked_lines_kernel<kMaskedSum>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((masked_lines_kernel<kMaskedLineEmit>), grid, block, 0, st, a);
    return hipGetLastError();
}

}  // namespace ss

namespace ssh {
namespace {

// The choice of include/sliceslice_hip_masked.h: `mask` may be NULL (all 0xFF).
void choose_masked_filter(const uint8_t *value, const uint8_t *mask, size_t n, const uint64_t *hist, size_t *anchor, size_t *distance)
{
    const ByteCost cost(nullptr);
    std::vector<uint64_t> c(n, 0);
    std::vector<uint8_t> usable(n, 0);
    for (size_t i = 0; i < n; ++i) {
        const uint8_t m = mask ? mask[i] : 0xFF, v = value[i] & m;
        usable[i] = m != 0;
        uint64_t sum = 0, seen = 0, accepted = 0;
        for (int b = 0; b < 256; ++b) {
            if (((uint8_t)b & m) != v) continue;
            ++accepted;
            sum += (uint64_t)cost((uint8_t)b);
            if (hist) seen += hist[b];
        }
        if (hist) {                                     // ~8 * log2 of the accepted values' count, as ByteCost takes one value's
            const uint64_t k = seen + 1;
            const int lg = 63 - __builtin_clzll(k);
            const int frac = lg >= 3 ? (int)((k >> (lg - 3)) & 7) : (int)((k << (3 - lg)) & 7);
            sum = (uint64_t)(8 * lg + frac);
        }
        c[i] = sum + accepted;
    }
    size_t best_a = 0, best_d = 0;
    uint64_t best = ~0ull;
    bool pair = false;
    for (size_t i = 0; i < n; ++i) {
        if (!usable[i]) continue;
        for (size_t j = i + 1; j < n && j - i <= 16; ++j) {
            if (!usable[j]) continue;
            if (!pair || c[i] + c[j] < best) {
                pair = true;
                best = c[i] + c[j];
                best_a = i;
                best_d = j - i;
            }
        }
    }
    if (!pair) {                                        // one filter byte: the cheapest position that has a mask, else position 0
        for (size_t i = 0; i < n; ++i) {
            if (usable[i] && c[i] < best) {
                best = c[i];
                best_a = i;
            }
        }
    }
    *anchor = best_a;
    *distance = best_d;
}

int hex_digit(char ch)
{
    if (ch >= '0' && ch <= '9') return ch - '0';
    if (ch >= 'a' && ch <= 'f') return ch - 'a' + 10;
    if (ch >= 'A' && ch <= 'F') return ch - 'A' + 10;
    return -1;
}

// What every scan refuses, and the argument block of the view.  `waits`: the call waits for its stream.
int masked_args(const char *name, const ss_masked *p, const void *d_haystack, size_t len, bool waits, hipStream_t st, ss::MaskedArgs *a)
{
    if (!p) return fail(SS_ERR_ARGUMENT, "%s: the pattern is NULL", name);
    if (len && !d_haystack) return fail(SS_ERR_ARGUMENT, "%s: haystack is NULL", name);
    if (waits && stream_is_capturing(st)) return fail(SS_ERR_ARGUMENT, "%s waits for its stream and cannot be captured into a hipGraph", name);
    int dev = -1;
    HIP_TRY(hipGetDevice(&dev));
    if (dev != p->dev) return fail(SS_ERR_ARGUMENT, "%s: the pattern was made on device %d, the current device is %d", name, p->dev, dev);
    const uint8_t *hay = static_cast<const uint8_t *>(d_haystack);
    *a = ss::MaskedArgs{};
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
    a->v0x4 = p->value[p->a] * 0x01010101u;
    a->m0x4 = p->mask[p->a] * 0x01010101u;
    a->v1x4 = p->d ? p->value[p->a + p->d] * 0x01010101u : 0u;
    a->m1x4 = p->d ? p->mask[p->a + p->d] * 0x01010101u : 0u;
    if ((a->ntiles + ss::kSetTiles - 1) / ss::kSetTiles > 0x7fffffffull)
        return fail(SS_ERR_ARGUMENT, "%s: a haystack of %zu bytes needs more than 2^31 - 1 workgroups", name, len);
    return SS_OK;
}

bool accepts_byte(const ss_masked *p, int byte)
{
    for (uint32_t i = 0; i < p->n; ++i)
        if (((uint8_t)byte & p->mask[i]) == p->value[i]) return true;
    return false;
}

// Both line calls.  `find`: records are wanted (else the four output arguments are unused).
int lines_masked(const char *name, bool find, const ss_masked *p, const void *d_haystack, size_t len, int delimiter, void *hip_stream,
                 uint64_t *d_begin, uint64_t *d_end, uint64_t *d_number, uint64_t capacity, uint64_t *lines)
{
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    if (!lines) return fail(SS_ERR_ARGUMENT, "%s: lines is NULL", name);
    if (delimiter < 0 || delimiter > 255) return fail(SS_ERR_ARGUMENT, "delimiter %d is not a byte (0 .. 255)", delimiter);
    ss::MaskedArgs a;
    if (int rc = masked_args(name, p, d_haystack, len, true, st, &a)) return rc;
    if (len < p->n) {
        *lines = 0;
        return SS_OK;
    }
    const uint64_t parts = (a.ntiles + ss::kSetTiles - 1) / ss::kSetTiles;
    const uint64_t chunks = (parts + ss::kLineChunk - 1) / ss::kLineChunk;
    // [total, 32 bytes][LineSum x parts][LinePre x parts][LineSum x chunks][LinePre x chunks], as ss_needleset.hip lays it out
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
    HIP_TRY(ss::launch_masked_lines(a, ss::kMaskedSum, st));
    HIP_TRY(ss::launch_lines_chunks(sum, parts, csum, cpre, pre, false, st));
    const bool emit = find && capacity != 0 && (d_begin || d_end || d_number);
    const ss::CombineArgs ca = {csum, chunks, cpre, d_total, nullptr, len, emit ? d_begin : nullptr, emit ? d_end : nullptr,
                                emit ? d_number : nullptr, emit ? capacity : 0};
    HIP_TRY(ss::launch_lines_combine(ca, st));
    if (emit) {
        HIP_TRY(ss::launch_lines_chunks(sum, parts, csum, cpre, pre, true, st));
        a.begin = d_begin;
        a.end = d_end;
        a.number = d_number;
        a.capacity = capacity;
        HIP_TRY(ss::launch_masked_lines(a, ss::kMaskedLineEmit, st));
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

int ss_masked_parse_hex(const char *text, uint8_t *value, uint8_t *mask, size_t capacity, size_t *n)
{
    if (!text || !n) return fail(SS_ERR_ARGUMENT, "NULL argument");
    size_t count = 0;
    for (size_t i = 0; text[i] != '\0';) {
        if (text[i] == ' ' || text[i] == '\t') {
            ++i;
            continue;
        }
        uint8_t v = 0, m = 0;
        for (int half = 0; half < 2; ++half) {
            const char ch = text[i + (size_t)half];
            const int h = hex_digit(ch);
            if (ch == '\0') return fail(SS_ERR_ARGUMENT, "ss_masked_parse_hex: column %zu: the text ends inside a token of two characters", i + 2);
            if (h < 0 && ch != '?')
                return fail(SS_ERR_ARGUMENT, "ss_masked_parse_hex: column %zu: '%c' is neither a hex digit nor '?'", i + (size_t)half + 1, ch);
            v = (uint8_t)(v << 4 | (h < 0 ? 0 : h));
            m = (uint8_t)(m << 4 | (h < 0 ? 0 : 0xF));
        }
        if (count < capacity) {
            if (value) value[count] = v;
            if (mask) mask[count] = m;
        }
        ++count;
        i += 2;
    }
    *n = count;
    return SS_OK;
}

int ss_masked_choose_filter(const void *value, const void *mask, size_t n, const uint64_t *hist, size_t *anchor, size_t *distance)
{
    if (!value || !anchor || !distance) return fail(SS_ERR_ARGUMENT, "NULL argument");
    if (n == 0 || n > SS_MASKED_MAX_LEN) return fail(SS_ERR_ARGUMENT, "ss_masked_choose_filter: a pattern holds 1 .. %d bytes, not %zu", SS_MASKED_MAX_LEN, n);
    choose_masked_filter(static_cast<const uint8_t *>(value), static_cast<const uint8_t *>(mask), n, hist, anchor, distance);
    return SS_OK;
}

int ss_masked_new(const void *value, const void *mask, size_t n, ss_masked **pattern)
{
    if (!value || !pattern) return fail(SS_ERR_ARGUMENT, "NULL argument");
    if (n == 0 || n > SS_MASKED_MAX_LEN) return fail(SS_ERR_ARGUMENT, "ss_masked_new: a pattern holds 1 .. %d bytes, not %zu", SS_MASKED_MAX_LEN, n);
    ss_masked *p = new (std::nothrow) ss_masked;
    if (!p) return fail(SS_ERR_NOMEM, "ss_masked_new: out of memory");
    struct Guard {
        ss_masked *p;
        ~Guard() { if (p) ss_masked_free(p); }
    } guard{p};
    const uint8_t *v = static_cast<const uint8_t *>(value), *m = static_cast<const uint8_t *>(mask);
    const size_t nw = (n + 3) / 4;
    std::vector<uint32_t> tab;
    try {
        p->value.resize(n);
        p->mask.resize(n);
        tab.assign(2 * nw, 0u);
    } catch (const std::bad_alloc &) {
        return fail(SS_ERR_NOMEM, "ss_masked_new: out of memory");
    }
    for (size_t i = 0; i < n; ++i) {
        p->mask[i] = m ? m[i] : 0xFF;
        p->value[i] = v[i] & p->mask[i];
        tab[2 * (i / 4)] |= (uint32_t)p->value[i] << (8 * (i % 4));
        tab[2 * (i / 4) + 1] |= (uint32_t)p->mask[i] << (8 * (i % 4));
    }
    p->n = (uint32_t)n;
    size_t a = 0, d = 0;
    choose_masked_filter(p->value.data(), p->mask.data(), n, nullptr, &a, &d);
    p->a = (uint32_t)a;
    p->d = (uint32_t)d;
    HIP_TRY(hipGetDevice(&p->dev));
    const hipError_t e = hipMalloc(reinterpret_cast<void **>(&p->d_tab), tab.size() * 4);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        p->d_tab = nullptr;
        return fail(e == hipErrorOutOfMemory ? SS_ERR_NOMEM : SS_ERR_HIP, "ss_masked_new: %zu bytes for the tables: %s", tab.size() * 4, hipGetErrorString(e));
    }
    HIP_TRY(hipMemcpy(p->d_tab, tab.data(), tab.size() * 4, hipMemcpyHostToDevice));
    guard.p = nullptr;
    *pattern = p;
    return SS_OK;
}

void ss_masked_free(ss_masked *p)
{
    if (!p) return;
    if (p->d_tab) (void)hipFree(p->d_tab);
    delete p;
}

int ss_masked_info(const ss_masked *p, int delimiter, ss_masked_stats *stats)
{
    if (!p || !stats) return fail(SS_ERR_ARGUMENT, "NULL argument");
    if (delimiter > 255) return fail(SS_ERR_ARGUMENT, "delimiter %d is not a byte (0 .. 255)", delimiter);
    ss_masked_stats s = {p->n, p->a, p->d, 0, 0, 0, 0, 0};
    for (uint32_t i = 0; i < p->n; ++i) ++(p->mask[i] == 0xFF ? s.full : p->mask[i] == 0 ? s.wild : s.partial);
    s.accepts_delimiter = delimiter >= 0 && accepts_byte(p, delimiter) ? 1 : 0;
    *stats = s;
    return SS_OK;
}

int ss_count_masked_device_async(const ss_masked *p, const void *d_haystack, size_t len, void *hip_stream, uint64_t *d_count)
{
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    if (!d_count) return fail(SS_ERR_ARGUMENT, "ss_count_masked_device_async: d_count is NULL");
    ss::MaskedArgs a;
    if (int rc = masked_args("ss_count_masked_device_async", p, d_haystack, len, false, st, &a)) return rc;
    HIP_TRY(hipMemsetAsync(d_count, 0, sizeof(uint64_t), st));
    if (len < p->n) return SS_OK;
    a.total = d_count;
    HIP_TRY(ss::launch_masked_all(a, ss::kMaskedCount, st));
    return SS_OK;
}

int ss_count_masked_device(const ss_masked *p, const void *d_haystack, size_t len, void *hip_stream, uint64_t *count)
{
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    if (!count) return fail(SS_ERR_ARGUMENT, "ss_count_masked_device: count is NULL");
    ss::MaskedArgs a;
    if (int rc = masked_args("ss_count_masked_device", p, d_haystack, len, true, st, &a)) return rc;
    if (len < p->n) {
        *count = 0;
        return SS_OK;
    }
    ScratchLease lease;
    if (int rc = take_scratch(p->dev, sizeof(uint64_t), &lease.sc, st)) return rc;
    a.total = reinterpret_cast<uint64_t *>(lease.sc.d);
    HIP_TRY(hipMemsetAsync(a.total, 0, sizeof(uint64_t), st));
    HIP_TRY(ss::launch_masked_all(a, ss::kMaskedCount, st));
    HIP_TRY(hipMemcpyAsync(lease.sc.h, a.total, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    lease.done = true;
    *count = *lease.sc.h;
    return SS_OK;
}

int ss_find_all_masked_device(const ss_masked *p, const void *d_haystack, size_t len, void *hip_stream, uint64_t *d_offsets, uint64_t capacity,
                              uint64_t *total)
{
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    if (!total) return fail(SS_ERR_ARGUMENT, "ss_find_all_masked_device: total is NULL");
    if (capacity && !d_offsets) return fail(SS_ERR_ARGUMENT, "ss_find_all_masked_device: offsets are NULL with a capacity of %llu", (unsigned long long)capacity);
    ss::MaskedArgs a;
    if (int rc = masked_args("ss_find_all_masked_device", p, d_haystack, len, true, st, &a)) return rc;
    if (len < p->n) {
        *total = 0;
        return SS_OK;
    }
    const uint64_t parts = (a.ntiles + ss::kSetTiles - 1) / ss::kSetTiles;
    // [total u64][rank u64 x parts][occurrences u64 x parts]
    ScratchLease lease;
    if (int rc = take_scratch(p->dev, 8 + parts * 16, &lease.sc, st)) return rc;
    uint64_t *d_total = reinterpret_cast<uint64_t *>(lease.sc.d);
    uint64_t *d_rank = d_total + 1;
    a.wg = d_rank + parts;
    HIP_TRY(ss::launch_masked_all(a, ss::kMaskedCount, st));
    HIP_TRY(ss::launch_set_prefix(a.wg, parts, d_rank, d_total, st));
    if (capacity != 0) {
        a.wg_rank = d_rank;
        a.offsets = d_offsets;
        a.capacity = capacity;
        HIP_TRY(ss::launch_masked_all(a, ss::kMaskedEmit, st));
    }
    HIP_TRY(hipMemcpyAsync(lease.sc.h, d_total, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    lease.done = true;
    *total = *lease.sc.h;
    return SS_OK;
}

int ss_count_lines_masked_device(const ss_masked *p, const void *d_haystack, size_t len, int delimiter, void *hip_stream, uint64_t *lines)
{
    return lines_masked("ss_count_lines_masked_device", false, p, d_haystack, len, delimiter, hip_stream, nullptr, nullptr, nullptr, 0, lines);
}

int ss_find_lines_masked_device(const ss_masked *p, const void *d_haystack, size_t len, int delimiter, void *hip_stream, uint64_t *d_begin,
                                uint64_t *d_end, uint64_t *d_number, uint64_t capacity, uint64_t *lines)
{
    return lines_masked("ss_find_lines_masked_device", true, p, d_haystack, len, delimiter, hip_stream, d_begin, d_end, d_number, capacity,
                        lines);
}

}  // extern "C"
