// rewrite_launch.hpp - argument block and host-side entry point of the rewrite kernels (rewrite_kernels.hpp; defined and used in
// ss_rewrite.hip).
#pragma once
#include "runs_launch.hpp"

namespace ss {

constexpr int kRewriteSize = 0, kRewriteWrite = 1;              // runs_replace_kernel
constexpr uint32_t kRewriteMaxText = 4096;                      // SS_REWRITE_MAX_TEXT
constexpr uint32_t kRewriteWaveText = 16;                       // a longer text is copied by the whole wave, one begin at a time

struct RewriteArgs {
    RunsArgs r;                 // the view and the pattern; size: wg_b / wg_e are written; write: rank_b / rank_e are read
    uint64_t *wg_s;             // size: S = sum(e + 1) - sum(b) over the workgroup's selected ends and begins, in view coordinates
    const uint64_t *rank_s;     // write: the sum of S over the workgroups in front
    const uint32_t *rep;        // write: the text, device memory, 4-byte aligned, readable up to the next multiple of 4
    uint32_t rep_len;
    uint8_t *out;               // write
    uint64_t out_len;           // write: no store reaches out[out_len]
};

// ceil(ntiles / kSetTiles) workgroups of kBlock lanes
hipError_t launch_runs_replace(const RewriteArgs &a, int mode, hipStream_t st);

}  // namespace ss
