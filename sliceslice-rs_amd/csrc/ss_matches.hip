// ss_matches.hip - every occurrence of a needle (include/sliceslice_hip_matches.h): ss_count_device / _async, ss_find_all_device.
// NOT in libsliceslice_hip.so: libsliceslice_hip_matches.so holds the product's objects plus this file and scan_inst_all.hip.
//
// The scan is the find kernels' filter and verification with no early exit (scan_tiles<..., ALL = true>, scan_kernels.hpp):
//   count        one launch; each workgroup adds its count to one 64-bit word (a device-scope atomic, only when it has matches).
//   find_all     a count pass that writes one count per workgroup, the exclusive prefix sum of those counts (one workgroup), and an
//                emit pass over the same grid in which only the workgroups that hold one of the first `capacity` matches re-read
//                their tiles and write their offsets at their rank.  Workgroups take contiguous runs of tiles, so workgroup order is
//                address order and the offsets land sorted.
// The launch shape is the static one of an untuned search (plan_static, which ss_lines.hip uses too; ss_scan.hip, enqueue_scan with
// autotune off); the census is neither started nor read, so a searcher's tuning state is the same before and after these calls, and
// the answers cannot depend on it.
#include "ss_internal.hpp"

#include "../../include/sliceslice_hip_matches.h"
#include "matches_host.hpp"
#include "matches_scratch.hpp"

namespace ssh {

// (matches_host.hpp)
int plan_static(const ss_searcher *s, PerDevice *pd, const void *d_hay, size_t len, StaticPlan *out)
{
    fill_problem(s, pd->d_needle, d_hay, len, 0, &out->pr, &out->ps, nullptr);
    const int occ = guess_workgroups_per_cu(s, out->pr, out->ps);
    out->mode = out->pr.d == 0 ? 0 : 2;
    out->one_byte = out->ps.one_byte;
    out->q = (int)((out->ps.position % 16) / 4);
    out->ntiles = (out->pr.npieces + kPiecesPerTile - 1) / kPiecesPerTile;
    uint64_t tpb = 0, blocks = 0;
    if (int rc = launch_grid(pd->dev, out->mode, out->ntiles, &tpb, &blocks)) return rc;
    out->shape = {(unsigned)blocks, ss::kBlock, tpb, occupancy_pad(occ, ss::kBlock)};
    return SS_OK;
}

int check_common_args(const ss_searcher *s, const void *d_haystack, size_t len, const void *out)
{
    if (!s || !out) return fail(SS_ERR_ARGUMENT, "NULL argument");
    if (len && !d_haystack) return fail(SS_ERR_ARGUMENT, "haystack is NULL");
    return SS_OK;
}

namespace {

// (the call-owned scratch - Scratch, take_scratch, ScratchLease: matches_scratch.hpp, shared with ss_matches_batched.hip)

int launch_all(ss::ScanAllFn scan, const StaticPlan &al, hipStream_t st, const ss::AllArgs &aa, uint32_t bound)
{
    if (!scan(al.pr, al.q, al.mode, al.one_byte, al.shape, st, aa, bound))
        return fail(SS_ERR_ARGUMENT, "no all-matches kernel for mode %d, window %d", al.mode, al.q);
    HIP_TRY(hipGetLastError());
    return SS_OK;
}

}  // namespace

// (matches_host.hpp: `scan` is launch_scan_all, its case-folding twin for ss_nocase.hip, or a whole-word scan with its `bound`)
int count_device_async_with(ss::ScanAllFn scan, const ss_searcher *s, const void *d_haystack, size_t len, void *hip_stream,
                            uint64_t *d_count, uint32_t bound)
{
    if (int rc = check_common_args(s, d_haystack, len, d_count)) return rc;
    SearchGate gate(s);                                  // set_filter* are refused while this call runs
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    PerDevice *pd = nullptr;
    if (int rc = get_per_device(s, &pd)) return rc;
    s->used_async.store(true, std::memory_order_release);
    if (s->n == 0) {                                     // len + 1 empty matches
        HIP_TRY(ss::launch_store_u64(d_count, (uint64_t)len + 1, st));
        return SS_OK;
    }
    HIP_TRY(hipMemsetAsync(d_count, 0, sizeof(uint64_t), st));
    if (len < s->n) return SS_OK;
    StaticPlan al;
    if (int rc = plan_static(s, pd, d_haystack, len, &al)) return rc;
    const ss::AllArgs aa = {d_count, nullptr, nullptr, nullptr, 0, ss::kAllCount};
    return launch_all(scan, al, st, aa, bound);
}

int count_device_with(ss::ScanAllFn scan, const ss_searcher *s, const void *d_haystack, size_t len, void *hip_stream, uint64_t *count,
                      uint32_t bound)
{
    if (int rc = check_common_args(s, d_haystack, len, count)) return rc;
    SearchGate gate(s);
    if (s->n == 0) { *count = (uint64_t)len + 1; return SS_OK; }
    if (len < s->n) { *count = 0; return SS_OK; }
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    PerDevice *pd = nullptr;
    if (int rc = get_per_device(s, &pd)) return rc;
    StaticPlan al;
    if (int rc = plan_static(s, pd, d_haystack, len, &al)) return rc;
    ScratchLease lease;
    if (int rc = take_scratch(pd->dev, sizeof(uint64_t), &lease.sc, st)) return rc;
    uint64_t *d_total = reinterpret_cast<uint64_t *>(lease.sc.d);
    HIP_TRY(hipMemsetAsync(d_total, 0, sizeof(uint64_t), st));
    const ss::AllArgs aa = {d_total, nullptr, nullptr, nullptr, 0, ss::kAllCount};
    if (int rc = launch_all(scan, al, st, aa, bound)) return rc;
    HIP_TRY(hipMemcpyAsync(lease.sc.h, d_total, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    lease.done = true;
    *count = *lease.sc.h;
    return SS_OK;
}

int find_all_device_with(ss::ScanAllFn scan, const ss_searcher *s, const void *d_haystack, size_t len, void *hip_stream,
                         uint64_t *d_offsets, uint64_t capacity, uint64_t *count, uint32_t bound)
{
    if (int rc = check_common_args(s, d_haystack, len, count)) return rc;
    if (capacity && !d_offsets) return fail(SS_ERR_ARGUMENT, "offsets are NULL with a capacity of %llu", (unsigned long long)capacity);
    SearchGate gate(s);
    if (len < s->n) { *count = 0; return SS_OK; }
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    if (s->n == 0) {                                     // offsets 0 .. len
        const uint64_t total = (uint64_t)len + 1;
        if (capacity) {
            HIP_TRY(ss::launch_iota(d_offsets, total < capacity ? total : capacity, st));
            HIP_TRY(hipStreamSynchronize(st));
        }
        *count = total;
        return SS_OK;
    }
    PerDevice *pd = nullptr;
    if (int rc = get_per_device(s, &pd)) return rc;
    StaticPlan al;
    if (int rc = plan_static(s, pd, d_haystack, len, &al)) return rc;
    const uint64_t blocks = al.shape.blocks;
    // [total u64][rank u64 x blocks][count u32 x blocks]
    ScratchLease lease;
    if (int rc = take_scratch(pd->dev, 8 + blocks * 12, &lease.sc, st)) return rc;
    uint64_t *d_total = reinterpret_cast<uint64_t *>(lease.sc.d);
    uint64_t *d_rank = d_total + 1;
    uint32_t *d_wg = reinterpret_cast<uint32_t *>(d_rank + blocks);
    const ss::AllArgs counting = {nullptr, d_wg, nullptr, nullptr, 0, ss::kAllCountPerWorkgroup};
    if (int rc = launch_all(scan, al, st, counting, bound)) return rc;
    HIP_TRY(ss::launch_prefix(d_wg, blocks, d_rank, d_total, st));
    if (capacity) {
        const ss::AllArgs emitting = {nullptr, d_wg, d_rank, d_offsets, capacity, ss::kAllEmit};
        if (int rc = launch_all(scan, al, st, emitting, bound)) return rc;
    }
    HIP_TRY(hipMemcpyAsync(lease.sc.h, d_total, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    lease.done = true;
    *count = *lease.sc.h;
    return SS_OK;
}

}  // namespace ssh

using namespace ssh;

extern "C" {

int ss_count_device_async(const ss_searcher *s, const void *d_haystack, size_t len, void *hip_stream, uint64_t *d_count)
{
    return count_device_async_with(ss::launch_scan_all, s, d_haystack, len, hip_stream, d_count);
}

int ss_count_device(const ss_searcher *s, const void *d_haystack, size_t len, void *hip_stream, uint64_t *count)
{
    return count_device_with(ss::launch_scan_all, s, d_haystack, len, hip_stream, count);
}

int ss_find_all_device(const ss_searcher *s, const void *d_haystack, size_t len, void *hip_stream, uint64_t *d_offsets,
                       uint64_t capacity, uint64_t *count)
{
    return find_all_device_with(ss::launch_scan_all, s, d_haystack, len, hip_stream, d_offsets, capacity, count);
}

}  // extern "C"
