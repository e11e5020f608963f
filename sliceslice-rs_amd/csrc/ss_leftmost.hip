// ss_leftmost.hip - the leftmost-longest, non-overlapping occurrences of a needle set and the haystack with each of them replaced by
// its needle's own text (include/sliceslice_hip_leftmost.h): ss_select_leftmost_device, ss_count_leftmost_set_device,
// ss_find_all_leftmost_set_device, ss_replace_set_device and ss_needle_set_lengths.  NOT in the other libraries:
// libsliceslice_hip_leftmost.so holds the output library's objects plus this file.
//
// ss_select_leftmost_device is the primitive: the selection over a list of (offset, length) entries in blocks of SS_LEFTMOST_BLOCK
// (leftmost_kernels.hpp: the largest length, the block kernel, the chain kernel, the prefix over the blocks' selections and - when
// something is wanted - the emit kernel over the blocks below the capacity).  The haystack calls run the set's own count, the set's
// find call into temporary device memory through their public entry points, and the primitive with the lengths taken from a
// per-rank table.  ss_replace_set_device adds the selections' output starts and the copy pass over the output's chunks.  Every
// refusal of a model is the model's.
#include "ss_internal.hpp"

#include "../../include/sliceslice_hip_leftmost.h"
#include "leftmost_host.hpp"
#include "leftmost_kernels.hpp"
#include "matches_scratch.hpp"
#include "needleset_host.hpp"

namespace ss {

hipError_t launch_leftmost_longest(const LeftmostArgs &a, hipStream_t st)
{
    hipLaunchKernelGGL(leftmost_longest_kernel, dim3((unsigned)a.blocks), dim3(kLeftmostThreads), 0, st, a);
    if (hipError_t e = hipGetLastError()) return e;
    hipLaunchKernelGGL(leftmost_longest_final_kernel, dim3(1), dim3(kLeftmostThreads), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_leftmost_block(const LeftmostArgs &a, hipStream_t st)
{
    hipLaunchKernelGGL(leftmost_block_kernel, dim3((unsigned)a.blocks), dim3(kLeftmostThreads), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_leftmost_chain(const LeftmostArgs &a, hipStream_t st)
{
    hipLaunchKernelGGL(leftmost_chain_kernel, dim3(1), dim3(kLeftmostThreads), 0, st, a);
    if (hipError_t e = hipGetLastError()) return e;
    hipLaunchKernelGGL((prefix_kernel<uint64_t>), dim3(1), dim3(kPrefixThreads), 0, st, (const uint64_t *)a.cnt, a.blocks, a.rank, a.total);
    return hipGetLastError();
}

hipError_t launch_leftmost_emit(const LeftmostArgs &a, hipStream_t st)
{
    hipLaunchKernelGGL(leftmost_emit_kernel, dim3((unsigned)a.blocks), dim3(kLeftmostThreads), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_leftmost_deltas(const LeftmostReplaceArgs &a, hipStream_t st)
{
    hipLaunchKernelGGL(leftmost_deltas_kernel, dim3((unsigned)a.blocks), dim3(kLeftmostThreads), 0, st, a);
    if (hipError_t e = hipGetLastError()) return e;
    hipLaunchKernelGGL((prefix_kernel<uint64_t>), dim3(1), dim3(kPrefixThreads), 0, st, (const uint64_t *)a.sum, a.blocks, a.rank, a.total);
    return hipGetLastError();
}

hipError_t launch_leftmost_starts(const LeftmostReplaceArgs &a, hipStream_t st)
{
    hipLaunchKernelGGL(leftmost_starts_kernel, dim3((unsigned)a.blocks), dim3(kLeftmostThreads), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_leftmost_copy(const LeftmostReplaceArgs &a, hipStream_t st)
{
    hipLaunchKernelGGL(leftmost_copy_kernel, dim3((unsigned)a.chunks), dim3(kLeftmostCopyThreads), 0, st, a);
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

// the length of every rank, from the set's own tables (0: the empty needle)
std::vector<uint64_t> rank_lengths(const ss::SetTables &t)
{
    std::vector<uint64_t> lens((size_t)t.distinct, 0);
    for (uint32_t b = 0; b < 256 && b < t.rank1.size(); ++b)
        if (t.rank1[b] != ss::kSetNoSlot && t.rank1[b] < lens.size()) lens[t.rank1[b]] = 1;
    for (uint32_t r : t.rank2)
        if (r < lens.size()) lens[r] = 2;
    for (size_t e = 0; e < t.erank.size(); ++e)
        if (t.erank[e] < lens.size()) lens[t.erank[e]] = t.entry[e].len;
    return lens;
}

// The selection in two steps, so that a caller can size its arrays between them: run() gives the total and keeps the records,
// emit() writes the leftmost `capacity` selections.  rec: 8 bytes per entry of the call's own; [total: 32 bytes][cnt x blocks]
// [rank x blocks][head x blocks][entry x blocks] from the free list.  Neither step waits for the stream but run()'s read of the total.
struct Selection {
    ss::LeftmostArgs a = {};
    DeviceBytes rec;
    ScratchLease lease;

    int run(const char *name, int dev, hipStream_t st, uint64_t *selected)
    {
        *selected = 0;
        a.blocks = (a.count + SS_LEFTMOST_BLOCK - 1) / SS_LEFTMOST_BLOCK;
        if (a.count > ss::kLeftmostExitMask || a.blocks > kGridMax)
            return fail(SS_ERR_ARGUMENT, "%s: %llu entries; a call takes fewer than 2^%d, in at most 2^31 - 1 blocks of %u", name,
                        (unsigned long long)a.count, ss::kLeftmostExitBits, (unsigned)SS_LEFTMOST_BLOCK);
        if (int rc = rec.take(a.count * sizeof(uint64_t), name, "records of the selection")) return rc;
        if (int rc = take_scratch(dev, 32 + a.blocks * 24, &lease.sc, st)) return rc;
        uint64_t *w = reinterpret_cast<uint64_t *>(lease.sc.d);
        a.rec = reinterpret_cast<uint64_t *>(rec.d);
        a.total = w;
        a.cnt = w + 4;
        a.rank = a.cnt + a.blocks;
        a.head = reinterpret_cast<uint32_t *>(a.rank + a.blocks);
        a.entry = a.head + a.blocks;
        HIP_TRY(ss::launch_leftmost_longest(a, st));
        HIP_TRY(ss::launch_leftmost_block(a, st));
        HIP_TRY(ss::launch_leftmost_chain(a, st));
        HIP_TRY(hipMemcpyAsync(lease.sc.h, a.total, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        *selected = *lease.sc.h;
        return SS_OK;
    }

    int emit(hipStream_t st, uint64_t *d_selected, uint64_t *d_which, uint32_t *d_ranks, uint64_t capacity)
    {
        a.out = d_selected;
        a.which = d_which;
        a.out_ranks = d_ranks;
        a.capacity = (d_selected || d_which || d_ranks) ? capacity : 0;
        if (a.capacity != 0) HIP_TRY(ss::launch_leftmost_emit(a, st));
        return SS_OK;
    }

    // behind the caller's last wait for the stream: nothing is using the scratch any more
    void finished() { lease.done = true; }
};

// What the haystack calls check themselves; everything else is the set's count call's to refuse.
int check_set_call(const char *name, const ss_needle_set *set, const void *count)
{
    if (!set) return fail(SS_ERR_ARGUMENT, "%s: the set is NULL", name);
    if (!count) return fail(SS_ERR_ARGUMENT, "%s: a result pointer is NULL", name);
    return SS_OK;
}

// The set's pairs in temporary device memory ([offset x taken][rank x taken], 12 bytes per pair) and the lengths of the ranks beside
// them.  count == 0: there is none, and nothing was taken.
struct Pairs {
    DeviceBytes mem, table;
    uint64_t taken = 0, count = 0;

    int list(const char *name, const ss_needle_set *set, const void *d_haystack, size_t len, unsigned how, void *hip_stream,
             const std::vector<uint64_t> &lens)
    {
        hipStream_t st = static_cast<hipStream_t>(hip_stream);
        if (int rc = ss_count_set_device(set, d_haystack, len, how, hip_stream, nullptr, &taken)) return rc;
        if (taken == 0) return SS_OK;
        if (taken > ss::kLeftmostExitMask)
            return fail(SS_ERR_ARGUMENT, "%s: %llu pairs; a call takes fewer than 2^%d", name, (unsigned long long)taken, ss::kLeftmostExitBits);
        if (int rc = mem.take(taken * 12, name, "pairs of the set")) return rc;
        if (int rc = table.take(lens.size() * sizeof(uint64_t), name, "lengths of the ranks")) return rc;
        HIP_TRY(hipMemcpyAsync(table.d, lens.data(), lens.size() * sizeof(uint64_t), hipMemcpyHostToDevice, st));
        uint64_t again = 0;
        if (int rc = ss_find_all_set_device(set, d_haystack, len, how, hip_stream, reinterpret_cast<uint64_t *>(mem.d),
                                            reinterpret_cast<uint32_t *>(mem.d + taken * 8), taken, &again))
            return rc;
        count = again < taken ? again : taken;                  // (the haystack changed under the call: stay inside what was written)
        return SS_OK;
    }

    void describe(ss::LeftmostArgs *a) const
    {
        a->offsets = reinterpret_cast<const uint64_t *>(mem.d);
        a->lengths = nullptr;
        a->ranks = reinterpret_cast<const uint32_t *>(mem.d + taken * 8);
        a->rank_len = reinterpret_cast<const uint64_t *>(table.d);
        a->count = count;
    }
};

// The count and the find call (both arrays NULL or capacity 0: the count).
int find_all_leftmost(const char *name, const ss_needle_set *set, const void *d_haystack, size_t len, unsigned how, void *hip_stream,
                      uint64_t *d_offsets, uint32_t *d_ranks, uint64_t capacity, uint64_t *count)
{
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    if (int rc = check_set_call(name, set, count)) return rc;
    const std::vector<uint64_t> lens = rank_lengths(set->host);
    Pairs pairs;
    if (int rc = pairs.list(name, set, d_haystack, len, how, hip_stream, lens)) return rc;
    *count = 0;
    if (pairs.count == 0) return SS_OK;
    Selection sel;
    pairs.describe(&sel.a);
    uint64_t total = 0;
    if (int rc = sel.run(name, set->dev, st, &total)) return rc;
    if (int rc = sel.emit(st, d_offsets, nullptr, d_ranks, capacity)) return rc;
    HIP_TRY(hipStreamSynchronize(st));
    sel.finished();
    *count = total;
    return SS_OK;
}

}  // namespace
}  // namespace ssh

using namespace ssh;

extern "C" {

int ss_needle_set_lengths(const ss_needle_set *set, uint64_t *lengths)
{
    if (!set || !lengths) return fail(SS_ERR_ARGUMENT, "NULL argument");
    const std::vector<uint64_t> lens = rank_lengths(set->host);
    std::copy(lens.begin(), lens.end(), lengths);
    return SS_OK;
}

int ss_select_leftmost_device(const ss_needle_set *set, const uint64_t *d_offsets, const uint64_t *d_lengths, uint64_t count, void *hip_stream,
                              uint64_t *d_selected, uint64_t *d_which, uint64_t capacity, uint64_t *selected)
{
    const char *name = "ss_select_leftmost_device";
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    if (int rc = check_set_call(name, set, selected)) return rc;
    if (count != 0 && (!d_offsets || !d_lengths))
        return fail(SS_ERR_ARGUMENT, "%s: d_offsets or d_lengths is NULL and count is %llu", name, (unsigned long long)count);
    if ((d_selected && d_selected == d_offsets) || (d_which && (d_which == d_offsets || d_which == d_lengths)) ||
        (d_selected && d_selected == d_lengths) || (d_selected && d_selected == d_which))
        return fail(SS_ERR_ARGUMENT, "%s: d_selected or d_which is one of the other arrays; the selection is not made in place", name);
    if (stream_is_capturing(st)) return fail(SS_ERR_ARGUMENT, "%s waits for its stream and cannot be captured into a hipGraph", name);
    int dev = -1;
    HIP_TRY(hipGetDevice(&dev));
    if (dev != set->dev) return fail(SS_ERR_ARGUMENT, "%s: the set was made on device %d, the current device is %d", name, set->dev, dev);
    if (count > ss::kLeftmostExitMask)
        return fail(SS_ERR_ARGUMENT, "%s: %llu entries; a call takes fewer than 2^%d", name, (unsigned long long)count, ss::kLeftmostExitBits);
    *selected = 0;
    if (count == 0) return SS_OK;
    Selection sel;
    sel.a.offsets = d_offsets;
    sel.a.lengths = d_lengths;
    sel.a.count = count;
    uint64_t total = 0;
    if (int rc = sel.run(name, set->dev, st, &total)) return rc;
    if (int rc = sel.emit(st, d_selected, d_which, nullptr, capacity)) return rc;
    HIP_TRY(hipStreamSynchronize(st));
    sel.finished();
    *selected = total;
    return SS_OK;
}

int ss_count_leftmost_set_device(const ss_needle_set *set, const void *d_haystack, size_t len, unsigned how, void *hip_stream, uint64_t *count)
{
    return find_all_leftmost("ss_count_leftmost_set_device", set, d_haystack, len, how, hip_stream, nullptr, nullptr, 0, count);
}

int ss_find_all_leftmost_set_device(const ss_needle_set *set, const void *d_haystack, size_t len, unsigned how, void *hip_stream,
                                    uint64_t *d_offsets, uint32_t *d_ranks, uint64_t capacity, uint64_t *count)
{
    return find_all_leftmost("ss_find_all_leftmost_set_device", set, d_haystack, len, how, hip_stream, d_offsets, d_ranks, capacity, count);
}

int ss_replace_set_device(const ss_needle_set *set, const void *d_haystack, size_t len, unsigned how, const void *const *replacements,
                          const size_t *replacement_lens, uint32_t needles, void *hip_stream, void *d_out, uint64_t out_capacity,
                          uint64_t *out_len, uint64_t *count)
{
    const char *name = "ss_replace_set_device";
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    if (int rc = check_set_call(name, set, count)) return rc;
    if (!out_len) return fail(SS_ERR_ARGUMENT, "%s: a result pointer is NULL", name);
    if ((uint64_t)needles != set->host.needles)
        return fail(SS_ERR_ARGUMENT, "%s: %u replacements for a set of %llu needles", name, needles, (unsigned long long)set->host.needles);
    if (needles != 0 && (!replacements || !replacement_lens)) return fail(SS_ERR_ARGUMENT, "%s: replacements or replacement_lens is NULL", name);
    for (uint32_t k = 0; k < needles; ++k)
        if (replacement_lens[k] != 0 && !replacements[k])
            return fail(SS_ERR_ARGUMENT, "%s: replacement %u is NULL and its length is %zu", name, k, replacement_lens[k]);
    std::vector<uint32_t> owner;
    const int64_t bad = rank_replacements(set->host.rank_of.data(), needles, replacements, replacement_lens, (size_t)set->host.distinct, &owner);
    if (bad >= 0)
        return fail(SS_ERR_ARGUMENT, "%s: needle %lld shares its rank with an earlier needle (equal, or equal after the set's fold) and carries another replacement",
                    name, (long long)bad);
    const uintptr_t h0 = reinterpret_cast<uintptr_t>(d_haystack), o0 = reinterpret_cast<uintptr_t>(d_out);
    if (d_out && d_haystack && len != 0 && out_capacity != 0 && o0 < h0 + len && h0 < o0 + out_capacity)
        return fail(SS_ERR_ARGUMENT, "%s: d_out[0, %llu) intersects the haystack; the replacement is not made in place", name,
                    (unsigned long long)out_capacity);
    // the per-rank table and the blob of replacement texts, padded for the copy pass's 16-byte loads
    const std::vector<uint64_t> lens = rank_lengths(set->host);
    std::vector<uint8_t> upload(lens.size() * sizeof(ss::LeftmostRank));
    uint64_t longest = 0;
    for (size_t r = 0; r < lens.size(); ++r) {
        ss::LeftmostRank row = {lens[r], upload.size() - lens.size() * sizeof(ss::LeftmostRank), 0};
        if (owner[r] != kLeftmostNoNeedle) {
            row.rep_len = replacement_lens[owner[r]];
            const uint8_t *text = static_cast<const uint8_t *>(replacements[owner[r]]);
            if (row.rep_len) upload.insert(upload.end(), text, text + row.rep_len);
            if (row.rep_len > longest) longest = row.rep_len;
        }
        std::memcpy(upload.data() + r * sizeof(ss::LeftmostRank), &row, sizeof(row));
    }
    upload.insert(upload.end(), ss::kLeftmostBlobPad, 0);
    // the selection: every refusal of `how`, of the set and of the stream is the set's count call's
    Pairs pairs;
    if (int rc = pairs.list(name, set, d_haystack, len, how, hip_stream, lens)) return rc;
    Selection sel;
    uint64_t nsel = 0;
    if (pairs.count != 0) {
        pairs.describe(&sel.a);
        if (int rc = sel.run(name, set->dev, st, &nsel)) return rc;
    }
    ss::LeftmostReplaceArgs ra = {};
    ra.nsel = nsel;
    ra.blocks = (nsel + SS_LEFTMOST_BLOCK - 1) / SS_LEFTMOST_BLOCK;
    DeviceBytes chosen, tables;
    ScratchLease lease;
    uint64_t delta = 0;
    if (nsel != 0) {
        // [offset x nsel][start x nsel][rank x nsel]; scratch [total: 32 bytes][sum x blocks][rank x blocks]
        if (int rc = chosen.take(nsel * 20, name, "selected occurrences")) return rc;
        if (int rc = tables.take(upload.size(), name, "replacements")) return rc;
        if (int rc = take_scratch(set->dev, 32 + ra.blocks * 16, &lease.sc, st)) return rc;
        uint64_t *d_sel = reinterpret_cast<uint64_t *>(chosen.d);
        uint32_t *d_sel_rank = reinterpret_cast<uint32_t *>(chosen.d + nsel * 16);
        if (int rc = sel.emit(st, d_sel, nullptr, d_sel_rank, nsel)) return rc;
        HIP_TRY(hipMemcpyAsync(tables.d, upload.data(), upload.size(), hipMemcpyHostToDevice, st));
        uint64_t *w = reinterpret_cast<uint64_t *>(lease.sc.d);
        ra.sel = d_sel;
        ra.starts = d_sel + nsel;
        ra.sel_rank = d_sel_rank;
        ra.table = reinterpret_cast<const ss::LeftmostRank *>(tables.d);
        ra.blob = tables.d + lens.size() * sizeof(ss::LeftmostRank);
        ra.total = w;
        ra.sum = w + 4;
        ra.rank = ra.sum + ra.blocks;
        HIP_TRY(ss::launch_leftmost_deltas(ra, st));
        HIP_TRY(ss::launch_leftmost_starts(ra, st));
        HIP_TRY(hipMemcpyAsync(lease.sc.h, ra.total, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        delta = *lease.sc.h;
        sel.finished();
        lease.done = true;
    }
    uint64_t total = 0;
    if (!replaced_set_length(len, nsel, longest, delta, &total))
        return fail(SS_ERR_ARGUMENT, "%s: %llu occurrences replaced by up to %llu bytes each do not fit 64 bits", name, (unsigned long long)nsel,
                    (unsigned long long)longest);
    *count = nsel;
    *out_len = total;
    if (out_capacity < total || total == 0) return SS_OK;
    if (!d_out) return fail(SS_ERR_ARGUMENT, "%s: d_out is NULL and the output holds %llu bytes", name, (unsigned long long)total);
    const uint64_t mis = (uint64_t)(o0 & 15);
    ra.hay = static_cast<const uint8_t *>(d_haystack);
    ra.len = len;
    ra.out_base = static_cast<uint8_t *>(d_out) - mis;
    ra.out_lo = mis;
    ra.out_hi = mis + total;
    ra.chunks = (ra.out_hi + SS_OUTPUT_CHUNK - 1) / SS_OUTPUT_CHUNK;
    if (ra.chunks > kGridMax)
        return fail(SS_ERR_ARGUMENT, "%s: an output of %llu bytes needs %llu chunks of %u bytes; a grid holds 2^31 - 1", name,
                    (unsigned long long)total, (unsigned long long)ra.chunks, (unsigned)SS_OUTPUT_CHUNK);
    HIP_TRY(ss::launch_leftmost_copy(ra, st));
    HIP_TRY(hipStreamSynchronize(st));
    return SS_OK;
}

}  // extern "C"

