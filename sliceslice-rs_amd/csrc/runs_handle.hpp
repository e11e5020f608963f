// runs_handle.hpp - the run handle and the argument block of a view, shared by the translation units that scan runs (ss_runs.hip,
// ss_rewrite.hip).  A handle is host memory alone: the set, its ranges' constants and its bitmap travel in the kernels' argument
// block, so no call allocates device memory for the pattern.
#pragma once
#include "ss_internal.hpp"

#include "../../include/sliceslice_hip_runs.h"
#include "runs_launch.hpp"

struct ss_runs {
    uint64_t set[4];
    uint64_t min_len, max_len;
    uint32_t nranges_all;                   // the maximal ranges of the set
    uint32_t path;                          // 0: range tests, 1: the bitmap
    ss::RunsRange rg[ss::kRunsMaxRanges];
    int dev;
};

namespace ssh {

// What every scan refuses, and the argument block of the view.  `waits`: the call waits for its stream.
inline int runs_args(const char *name, const ss_runs *p, const void *d_haystack, size_t len, bool waits, hipStream_t st, ss::RunsArgs *ra)
{
    if (!p) return fail(SS_ERR_ARGUMENT, "%s: runs is NULL", name);
    if (len && !d_haystack) return fail(SS_ERR_ARGUMENT, "%s: haystack is NULL", name);
    if (waits && stream_is_capturing(st)) return fail(SS_ERR_ARGUMENT, "%s waits for its stream and cannot be captured into a hipGraph", name);
    int dev = -1;
    HIP_TRY(hipGetDevice(&dev));
    if (dev != p->dev) return fail(SS_ERR_ARGUMENT, "%s: the handle was made on device %d, the current device is %d", name, p->dev, dev);
    const uint8_t *hay = static_cast<const uint8_t *>(d_haystack);
    *ra = ss::RunsArgs{};
    ss::MaskedArgs *a = &ra->m;
    a->mis = (uint64_t)(reinterpret_cast<uintptr_t>(hay) & 15);
    a->base = hay - a->mis;
    a->hay = hay;
    a->len = len;
    a->nchunks = (a->mis + len + 15) / 16;
    a->ntiles = (a->nchunks + ss::kSetTileChunks - 1) / ss::kSetTileChunks;
    for (int r = 0; r < ss::kRunsMaxRanges; ++r) ra->rg[r] = p->rg[r];
    ra->nranges = p->path == 0 ? p->nranges_all : 0u;
    for (int k = 0; k < 4; ++k) {
        ra->bits[2 * k] = (uint32_t)p->set[k];
        ra->bits[2 * k + 1] = (uint32_t)(p->set[k] >> 32);
    }
    ra->min_len = (uint32_t)p->min_len;
    ra->max_len = (uint32_t)p->max_len;
    ra->look = (uint32_t)(p->max_len + 1 > p->min_len ? p->max_len + 1 : p->min_len);
    ra->simple = p->min_len == 1 && p->max_len == 0 ? 1u : 0u;
    if ((a->ntiles + ss::kSetTiles - 1) / ss::kSetTiles > 0x7fffffffull)
        return fail(SS_ERR_ARGUMENT, "%s: a haystack of %zu bytes needs more than 2^31 - 1 workgroups", name, len);
    return SS_OK;
}

}  // namespace ssh
