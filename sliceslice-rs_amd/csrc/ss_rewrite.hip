// ss_rewrite.hip - the selected runs of one byte class replaced or deleted on the device (include/sliceslice_hip_rewrite.h has THE
// RULE): ss_replace_runs_device.  NOT in the other libraries: libsliceslice_hip_rewrite.so holds the runs library's objects plus
// this file.
//
// Two passes over the haystack and no list of runs: the size pass leaves three words per workgroup, three prefix sums turn them into
// every workgroup's place in the output, the write pass puts every byte there.  The handle is ss_runs.hip's (runs_handle.hpp).
#include "ss_internal.hpp"

#include "../../include/sliceslice_hip_rewrite.h"
#include "matches_scratch.hpp"
#include "runs_handle.hpp"
#include "runs_host.hpp"
#include "rewrite_kernels.hpp"

namespace ss {

hipError_t launch_runs_replace(const RewriteArgs &a, int mode, hipStream_t st)
{
    const dim3 grid((unsigned)((a.r.m.ntiles + kSetTiles - 1) / kSetTiles)), block(kBlock);
    if (mode == kRewriteSize) hipLaunchKernelGGL((runs_replace_kernel<kRewriteSize>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((runs_replace_kernel<kRewriteWrite>), grid, block, 0, st, a);
    return hipGetLastError();
}

}  // namespace ss

using namespace ssh;

extern "C" {

int ss_replace_runs_device(const ss_runs *p, const void *d_haystack, size_t len, int delimiter, const void *replacement,
                           size_t replacement_len, void *hip_stream, void *d_out, uint64_t out_capacity, uint64_t *out_len, uint64_t *count)
{
    const char *name = "ss_replace_runs_device";
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    if (!p) return fail(SS_ERR_ARGUMENT, "%s: runs is NULL", name);
    if (!out_len || !count) return fail(SS_ERR_ARGUMENT, "%s: out_len or count is NULL", name);
    if (delimiter < -1 || delimiter > 255) return fail(SS_ERR_ARGUMENT, "%s: delimiter %d is neither -1 (none) nor a byte (0 .. 255)", name, delimiter);
    if (replacement_len > SS_REWRITE_MAX_TEXT)
        return fail(SS_ERR_ARGUMENT, "%s: a replacement of %zu bytes is longer than SS_REWRITE_MAX_TEXT (%d)", name, replacement_len, SS_REWRITE_MAX_TEXT);
    if (replacement_len && !replacement) return fail(SS_ERR_ARGUMENT, "%s: replacement is NULL and replacement_len is %zu", name, replacement_len);
    if (!d_out && out_capacity)
        return fail(SS_ERR_ARGUMENT, "%s: d_out is NULL with an out_capacity of %llu", name, (unsigned long long)out_capacity);
    const uintptr_t h0 = reinterpret_cast<uintptr_t>(d_haystack), o0 = reinterpret_cast<uintptr_t>(d_out);
    if (d_out && len != 0 && out_capacity != 0 && o0 < h0 + len && h0 < o0 + out_capacity)
        return fail(SS_ERR_ARGUMENT, "%s: d_out[0, %llu) intersects the haystack; the rewrite is not made in place", name,
                    (unsigned long long)out_capacity);
    ss::RewriteArgs wa = {};
    ss::RunsArgs &ra = wa.r;
    if (int rc = runs_args(name, p, d_haystack, len, true, st, &ra)) return rc;
    if (delimiter >= 0 && classes::set_has(p->set, (unsigned)delimiter)) {
        if (classes::set_size(p->set) == 1)
            return fail(SS_ERR_ARGUMENT, "%s: the set is only the delimiter 0x%02x, which is never a member here: nothing can match", name, delimiter);
        ra.bits[delimiter >> 5] &= ~(1u << (delimiter & 31));                   // the delimiter is never a member ...
        ra.nranges = 0;                                                         // ... on the bitmap path: the range constants hold it
    }
    if (len == 0) {
        *out_len = 0;
        *count = 0;
        return SS_OK;
    }
    const uint64_t parts = (ra.m.ntiles + ss::kSetTiles - 1) / ss::kSetTiles;
    // [begins, ends, S: their totals, u64 each][pad to 32][the text, 4,096 bytes][begins, ends, S, and their three ranks: u64 x parts each]
    ScratchLease lease;
    if (int rc = take_scratch(p->dev, 32 + ss::kRewriteMaxText + parts * 48, &lease.sc, st)) return rc;
    uint64_t *d_total = reinterpret_cast<uint64_t *>(lease.sc.d);
    uint32_t *d_rep = reinterpret_cast<uint32_t *>(lease.sc.d + 32);
    uint64_t *wg_b = reinterpret_cast<uint64_t *>(lease.sc.d + 32 + ss::kRewriteMaxText), *wg_e = wg_b + parts, *wg_s = wg_e + parts;
    uint64_t *rank_b = wg_s + parts, *rank_e = rank_b + parts, *rank_s = rank_e + parts;
    ra.wg_b = wg_b;
    ra.wg_e = wg_e;
    wa.wg_s = wg_s;
    wa.rep_len = (uint32_t)replacement_len;
    HIP_TRY(ss::launch_runs_replace(wa, ss::kRewriteSize, st));
    HIP_TRY(ss::launch_set_prefix(wg_b, parts, rank_b, d_total, st));
    HIP_TRY(ss::launch_set_prefix(wg_e, parts, rank_e, d_total + 1, st));
    HIP_TRY(ss::launch_set_prefix(wg_s, parts, rank_s, d_total + 2, st));
    uint64_t totals[3] = {0, 0, 0};
    HIP_TRY(hipMemcpyAsync(totals, d_total, sizeof(totals), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    // every selected run has closed at the view's end, so the third total is the sum of the selected runs' lengths
    const uint64_t runs = totals[0], removed = totals[2];
    uint64_t added = 0, total = 0;
    if (totals[1] != runs || removed > len || __builtin_mul_overflow(runs, (uint64_t)replacement_len, &added) ||
        __builtin_add_overflow((uint64_t)len - removed, added, &total)) {
        lease.done = true;
        if (totals[1] != runs || removed > len)
            return fail(SS_ERR_ARGUMENT, "%s: the haystack changed under the call (%llu begins, %llu ends)", name, (unsigned long long)runs,
                        (unsigned long long)totals[1]);
        return fail(SS_ERR_ARGUMENT, "%s: %llu runs replaced by %zu bytes each do not fit 64 bits", name, (unsigned long long)runs, replacement_len);
    }
    *count = runs;
    *out_len = total;
    if (out_capacity < total || total == 0) {
        lease.done = true;
        return SS_OK;
    }
    if (replacement_len) HIP_TRY(hipMemcpyAsync(d_rep, replacement, replacement_len, hipMemcpyHostToDevice, st));
    ra.rank_b = rank_b;
    ra.rank_e = rank_e;
    wa.rank_s = rank_s;
    wa.rep = d_rep;
    wa.out = static_cast<uint8_t *>(d_out);
    wa.out_len = total;
    HIP_TRY(ss::launch_runs_replace(wa, ss::kRewriteWrite, st));
    HIP_TRY(hipStreamSynchronize(st));
    lease.done = true;
    return SS_OK;
}

}  // extern "C"
