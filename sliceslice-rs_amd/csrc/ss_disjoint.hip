// ss_disjoint.hip - the non-overlapping occurrences of a needle and the haystack with each of them replaced
// (include/sliceslice_hip_disjoint.h): ss_select_disjoint_device, ss_count_disjoint_device, ss_find_all_disjoint_device and
// ss_replace_device.  NOT in the other libraries: libsliceslice_hip_disjoint.so holds the setmatches library's objects plus this file.
//
// ss_select_disjoint_device is the primitive: the greedy selection over a list of ascending offsets in blocks of SS_DISJOINT_BLOCK
// (disjoint_kernels.hpp: the block kernel, the chain kernel, the prefix over the blocks' selections and - when offsets are wanted -
// the emit kernel over the blocks below the capacity).  The count and the find call compute the needle's longest proper border on the
// host (disjoint_host.hpp).  Border 0: they ARE their model, called through its public entry point.  Border above 0: the model's
// count, the model's find call into temporary device memory, the primitive.  ss_replace_device takes the selected list the same
// way - for a border of 0 it is the model's list - stages the replacement in device memory and runs replace_kernel over the view.
// Every refusal of a model is the model's.
#include "ss_internal.hpp"

#include "../../include/sliceslice_hip_disjoint.h"
#include "disjoint_host.hpp"
#include "disjoint_kernels.hpp"
#include "matches_host.hpp"
#include "matches_scratch.hpp"

namespace ss {

hipError_t launch_disjoint_block(const DisjointArgs &a, hipStream_t st)
{
    hipLaunchKernelGGL(disjoint_block_kernel, dim3((unsigned)a.blocks), dim3(kDisjointThreads), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_disjoint_chain(const DisjointArgs &a, hipStream_t st)
{
    hipLaunchKernelGGL(disjoint_chain_kernel, dim3(1), dim3(kDisjointThreads), 0, st, a);
    if (hipError_t e = hipGetLastError()) return e;
    hipLaunchKernelGGL((prefix_kernel<uint64_t>), dim3(1), dim3(kPrefixThreads), 0, st, (const uint64_t *)a.cnt, a.blocks, a.rank, a.total);
    return hipGetLastError();
}

hipError_t launch_disjoint_emit(const DisjointArgs &a, hipStream_t st)
{
    hipLaunchKernelGGL(disjoint_emit_kernel, dim3((unsigned)a.blocks), dim3(kDisjointThreads), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_replace(const ReplaceArgs &a, hipStream_t st)
{
    hipLaunchKernelGGL(replace_kernel, dim3((unsigned)a.parts), dim3(kBlock), 0, st, a);
    return hipGetLastError();
}

}  // namespace ss

namespace ssh {
namespace {

constexpr uint64_t kGridMax = 0x7fffffffull;

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

// The primitive behind its argument checks.  rec: 8 bytes per offset of the call's own; [total: 32 bytes][cnt x blocks][rank x blocks]
// [head x blocks][entry x blocks] from the free list.
int select_disjoint(const char *name, const ss_searcher *s, const uint64_t *d_offsets, uint64_t count, uint64_t n, hipStream_t st,
                    uint64_t *d_selected, uint64_t capacity, uint64_t *selected)
{
    *selected = 0;
    if (count == 0) return SS_OK;
    ss::DisjointArgs a = {};
    a.offsets = d_offsets;
    a.count = count;
    a.n = n;
    a.blocks = (count + SS_DISJOINT_BLOCK - 1) / SS_DISJOINT_BLOCK;
    if (count > ss::kDisjointExitMask || a.blocks > kGridMax)
        return fail(SS_ERR_ARGUMENT, "%s: %llu offsets; a call takes fewer than 2^%d, in at most 2^31 - 1 blocks of %u", name,
                    (unsigned long long)count, ss::kDisjointExitBits, (unsigned)SS_DISJOINT_BLOCK);
    PerDevice *pd = nullptr;
    if (int rc = get_per_device(s, &pd)) return rc;
    DeviceBytes rec;
    if (int rc = rec.take(count * sizeof(uint64_t), name, "records of the selection")) return rc;
    ScratchLease lease;
    if (int rc = take_scratch(pd->dev, 32 + a.blocks * 24, &lease.sc, st)) return rc;
    uint64_t *w = reinterpret_cast<uint64_t *>(lease.sc.d);
    a.rec = reinterpret_cast<uint64_t *>(rec.d);
    a.total = w;
    a.cnt = w + 4;
    a.rank = a.cnt + a.blocks;
    a.head = reinterpret_cast<uint32_t *>(a.rank + a.blocks);
    a.entry = a.head + a.blocks;
    a.out = d_selected;
    a.capacity = d_selected ? capacity : 0;
    HIP_TRY(ss::launch_disjoint_block(a, st));
    HIP_TRY(ss::launch_disjoint_chain(a, st));
    if (a.capacity != 0) HIP_TRY(ss::launch_disjoint_emit(a, st));
    HIP_TRY(hipMemcpyAsync(lease.sc.h, a.total, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    lease.done = true;
    *selected = *lease.sc.h;
    return SS_OK;
}

// `how` of the three haystack calls, and the needle it allows
int check_disjoint_how(const char *name, const ss_searcher *s, unsigned how, bool replace)
{
    if (how & (SS_BOUND_LINE | SS_CONTEXT_INVERT))
        return fail(SS_ERR_ARGUMENT, "%s: how = 0x%x holds SS_BOUND_LINE or SS_CONTEXT_INVERT; occurrences know no line and have no complement", name, how);
    if (how & ~(SS_BOUND_WORD | SS_BOUND_NOCASE)) return fail(SS_ERR_ARGUMENT, "%s: how = 0x%x holds bits other than SS_BOUND_WORD | SS_BOUND_NOCASE", name, how);
    if (s && s->n == 0 && how != 0)
        return fail(SS_ERR_ARGUMENT, "%s: the empty needle takes how == 0 only; it has no case to fold and no neighbours to be a word between", name);
    if (s && s->n == 0 && replace)
        return fail(SS_ERR_ARGUMENT, "%s: the empty needle cannot be replaced; its len + 1 occurrences hold no byte", name);
    return SS_OK;
}

int model_count(const ss_searcher *s, const void *d_haystack, size_t len, unsigned how, void *hip_stream, uint64_t *count)
{
    if (how & SS_BOUND_WORD) return ss_count_bounded_device(s, d_haystack, len, how, hip_stream, count);
    if (how & SS_BOUND_NOCASE) return ss_count_nocase_device(s, d_haystack, len, hip_stream, count);
    return ss_count_device(s, d_haystack, len, hip_stream, count);
}

int model_find_all(const ss_searcher *s, const void *d_haystack, size_t len, unsigned how, void *hip_stream, uint64_t *d_offsets,
                   uint64_t capacity, uint64_t *count)
{
    if (how & SS_BOUND_WORD) return ss_find_all_bounded_device(s, d_haystack, len, how, hip_stream, d_offsets, capacity, count);
    if (how & SS_BOUND_NOCASE) return ss_find_all_nocase_device(s, d_haystack, len, hip_stream, d_offsets, capacity, count);
    return ss_find_all_device(s, d_haystack, len, hip_stream, d_offsets, capacity, count);
}

// The count and the find call (d_offsets NULL or capacity 0: the count).
int find_all_disjoint(const char *name, const ss_searcher *s, const void *d_haystack, size_t len, unsigned how, void *hip_stream,
                      uint64_t *d_offsets, uint64_t capacity, uint64_t *count)
{
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    if (int rc = check_common_args(s, d_haystack, len, count)) return rc;
    if (int rc = check_disjoint_how(name, s, how, false)) return rc;
    if (stream_is_capturing(st)) return fail(SS_ERR_ARGUMENT, "%s waits for its stream and cannot be captured into a hipGraph", name);
    if (!d_offsets) capacity = 0;
    if (longest_proper_border(s->needle.data(), s->n) == 0)             // no two occurrences overlap: the call IS its model
        return capacity ? model_find_all(s, d_haystack, len, how, hip_stream, d_offsets, capacity, count)
                        : model_count(s, d_haystack, len, how, hip_stream, count);
    uint64_t all = 0;
    if (int rc = model_count(s, d_haystack, len, how, hip_stream, &all)) return rc;
    *count = 0;
    if (all == 0) return SS_OK;
    DeviceBytes list;
    if (all > SIZE_MAX / sizeof(uint64_t)) return fail(SS_ERR_NOMEM, "%s: %llu overlapping occurrences are too many to list", name, (unsigned long long)all);
    if (int rc = list.take(all * sizeof(uint64_t), name, "overlapping occurrences")) return rc;
    uint64_t again = 0;
    if (int rc = model_find_all(s, d_haystack, len, how, hip_stream, reinterpret_cast<uint64_t *>(list.d), all, &again)) return rc;
    if (again < all) all = again;                                       // (the haystack changed under the call: stay inside what was written)
    return select_disjoint(name, s, reinterpret_cast<const uint64_t *>(list.d), all, s->n, st, d_offsets, capacity, count);
}

}  // namespace
}  // namespace ssh

using namespace ssh;

extern "C" {

int ss_select_disjoint_device(const ss_searcher *s, const uint64_t *d_offsets, uint64_t count, uint64_t n, void *hip_stream,
                              uint64_t *d_selected, uint64_t capacity, uint64_t *selected)
{
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    if (!s || !selected) return fail(SS_ERR_ARGUMENT, "NULL argument");
    if (n == 0) return fail(SS_ERR_ARGUMENT, "ss_select_disjoint_device: n is 0; occurrences of no length do not overlap");
    if (count != 0 && !d_offsets)
        return fail(SS_ERR_ARGUMENT, "ss_select_disjoint_device: d_offsets is NULL and count is %llu", (unsigned long long)count);
    if (d_selected && d_selected == d_offsets)
        return fail(SS_ERR_ARGUMENT, "ss_select_disjoint_device: d_selected is d_offsets; the selection is not made in place");
    if (stream_is_capturing(st))
        return fail(SS_ERR_ARGUMENT, "ss_select_disjoint_device waits for its stream and cannot be captured into a hipGraph");
    return select_disjoint("ss_select_disjoint_device", s, d_offsets, count, n, st, d_selected, capacity, selected);
}

int ss_count_disjoint_device(const ss_searcher *s, const void *d_haystack, size_t len, unsigned how, void *hip_stream, uint64_t *count)
{
    return find_all_disjoint("ss_count_disjoint_device", s, d_haystack, len, how, hip_stream, nullptr, 0, count);
}

int ss_find_all_disjoint_device(const ss_searcher *s, const void *d_haystack, size_t len, unsigned how, void *hip_stream,
                                uint64_t *d_offsets, uint64_t capacity, uint64_t *count)
{
    return find_all_disjoint("ss_find_all_disjoint_device", s, d_haystack, len, how, hip_stream, d_offsets, capacity, count);
}

int ss_replace_device(const ss_searcher *s, const void *d_haystack, size_t len, unsigned how, const void *replacement,
                      size_t replacement_len, void *hip_stream, void *d_out, uint64_t out_capacity, uint64_t *out_len, uint64_t *count)
{
    const char *name = "ss_replace_device";
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    if (!out_len) return fail(SS_ERR_ARGUMENT, "NULL argument");
    if (int rc = check_common_args(s, d_haystack, len, count)) return rc;
    if (int rc = check_disjoint_how(name, s, how, true)) return rc;
    if (replacement_len && !replacement) return fail(SS_ERR_ARGUMENT, "%s: replacement is NULL and replacement_len is %zu", name, replacement_len);
    if (stream_is_capturing(st)) return fail(SS_ERR_ARGUMENT, "%s waits for its stream and cannot be captured into a hipGraph", name);
    const uintptr_t h0 = reinterpret_cast<uintptr_t>(d_haystack), o0 = reinterpret_cast<uintptr_t>(d_out);
    if (d_out && len != 0 && out_capacity != 0 && o0 < h0 + len && h0 < o0 + out_capacity)
        return fail(SS_ERR_ARGUMENT, "%s: d_out[0, %llu) intersects the haystack; the replacement is not made in place", name,
                    (unsigned long long)out_capacity);
    // the selected list: the model's own where no two occurrences overlap
    const bool overlapping = longest_proper_border(s->needle.data(), s->n) != 0;
    uint64_t sel = 0;
    if (int rc = overlapping ? find_all_disjoint(name, s, d_haystack, len, how, hip_stream, nullptr, 0, &sel)
                             : model_count(s, d_haystack, len, how, hip_stream, &sel))
        return rc;
    uint64_t total = 0;
    if (!replaced_length(len, sel, s->n, replacement_len, &total))
        return fail(SS_ERR_ARGUMENT, "%s: %llu occurrences replaced by %zu bytes each do not fit 64 bits", name, (unsigned long long)sel, replacement_len);
    *count = sel;
    *out_len = total;
    if (out_capacity < total || total == 0) return SS_OK;
    if (!d_out) return fail(SS_ERR_ARGUMENT, "%s: d_out is NULL and the output holds %llu bytes", name, (unsigned long long)total);
    DeviceBytes list, rep;
    if (sel != 0) {
        if (sel > SIZE_MAX / sizeof(uint64_t)) return fail(SS_ERR_NOMEM, "%s: %llu occurrences are too many to list", name, (unsigned long long)sel);
        if (int rc = list.take(sel * sizeof(uint64_t), name, "selected occurrences")) return rc;
        uint64_t again = 0;
        if (int rc = overlapping ? find_all_disjoint(name, s, d_haystack, len, how, hip_stream, reinterpret_cast<uint64_t *>(list.d), sel, &again)
                                 : model_find_all(s, d_haystack, len, how, hip_stream, reinterpret_cast<uint64_t *>(list.d), sel, &again))
            return rc;
        if (again != sel)
            return fail(SS_ERR_ARGUMENT, "%s: the haystack changed under the call (%llu occurrences, then %llu)", name, (unsigned long long)sel,
                        (unsigned long long)again);
        if (replacement_len) {
            if (int rc = rep.take(replacement_len, name, "replacement")) return rc;
            HIP_TRY(hipMemcpyAsync(rep.d, replacement, replacement_len, hipMemcpyHostToDevice, st));
        }
    }
    const uint64_t mis = (uint64_t)(h0 & 15);
    ss::ReplaceArgs ra = {};
    ra.base = static_cast<const uint8_t *>(d_haystack) - mis;
    ra.lo = mis;
    ra.hi = mis + len;
    ra.parts = (ra.hi + SS_CONTEXT_PART_BYTES - 1) / SS_CONTEXT_PART_BYTES;
    if (ra.parts > kGridMax)
        return fail(SS_ERR_ARGUMENT, "a haystack of %zu bytes needs %llu parts of %u bytes; a grid holds 2^31 - 1", len, (unsigned long long)ra.parts,
                    (unsigned)SS_CONTEXT_PART_BYTES);
    ra.sel = reinterpret_cast<const uint64_t *>(list.d);
    ra.nsel = sel;
    ra.n = s->n;
    ra.rep = rep.d;
    ra.rep_len = replacement_len;
    ra.out = static_cast<uint8_t *>(d_out);
    if (len != 0) HIP_TRY(ss::launch_replace(ra, st));
    HIP_TRY(hipStreamSynchronize(st));
    return SS_OK;
}

}  // extern "C"
