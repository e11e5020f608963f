// runs_launch.hpp - argument block and host-side entry points of the run kernels (runs_kernels.hpp; defined and used in
// ss_runs.hip).
#pragma once
#include "masked_launch.hpp"
#include "runs_swar.hpp"

namespace ss {

constexpr int kRunsCount = 0, kRunsEmit = 1;                    // runs_all_kernel; the line kernel takes kMaskedSum / kMaskedLineEmit
constexpr uint32_t kRunsMaxLen = 4096;                          // SS_RUNS_MAX_LEN

struct RunsArgs {
    MaskedArgs m;               // the view (base, hay, mis, len, nchunks, ntiles), total, capacity and the line fields; the pattern
                                // fields are unused
    RunsRange rg[kRunsMaxRanges];
    uint32_t nranges;           // 0: the bitmap path
    uint32_t bits[8];           // the set: bit b & 31 of dword b >> 5 (line calls: without the delimiter); staged in LDS
    uint32_t min_len, max_len;  // max_len 0: none
    uint32_t look;              // max(min_len, max_len + 1): how far a begin looks ahead and an end looks back
    uint32_t simple;            // min_len == 1 and no maximum: every begin and every end is selected, nothing walks
    // count: the selected begins / ends of every workgroup (written; wg_e != NULL: ends are wanted at all); emit: read
    uint64_t *wg_b, *wg_e;
    const uint64_t *rank_b, *rank_e;    // emit: the selected begins / ends in front of every workgroup
    uint64_t *out_b, *out_e;            // emit: either may be NULL
};

// ceil(ntiles / kSetTiles) workgroups of kBlock lanes
hipError_t launch_runs_all(const RunsArgs &a, int mode, hipStream_t st);
hipError_t launch_runs_lines(const RunsArgs &a, int mode, hipStream_t st);

}  // namespace ss
