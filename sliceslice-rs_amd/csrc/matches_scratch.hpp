// matches_scratch.hpp - call-owned scratch of the all-matches calls (ss_matches.hip, ss_matches_batched.hip): workgroup counts,
// their prefix, descriptors, and a pinned word for the total that is read back.
// A call takes a buffer of its device from a free list (or allocates one) and hands it back when it is done with it, so two calls
// in flight - two threads, two streams - never share one.  Two ways of handing back:
//   * a call that WAITS for its stream sets ScratchLease::done once the wait has returned: nothing is using the buffer any more;
//   * a call that never waits (ss_count_batched) records the buffer's event behind its last launch (ScratchLease::release_on): the
//     next call on the SAME stream may take the buffer at once - launches of a stream run in order - any other call only once the
//     event has been reached.  "The same stream" is only ever concluded from two handles that callers passed: every caller names
//     the stream it launches on (the NULL stream is a stream like any other here: nothing orders a non-blocking stream behind it),
//     and hipStreamPerThread, one handle for a different stream in every thread, never counts as the same.
// A call that fails keeps its buffer out of the list (work it enqueued may still be running).
#pragma once
#include "ss_internal.hpp"

namespace ssh {

struct Scratch {
    int dev = -1;
    uint8_t *d = nullptr;
    size_t bytes = 0;
    uint64_t *h = nullptr;          // pinned: the total, read back
    hipEvent_t ev = nullptr;        // (calls that never wait) recorded behind the last launch that uses the buffer
    hipStream_t busy_on = nullptr;  // ... on this stream
    bool busy = false;              // `ev` has been recorded and not yet been seen reached
};
inline std::mutex g_scratch_mu;
inline std::vector<Scratch> g_scratch_free;

// `st`: the stream the caller is going to launch on (a buffer last used there without a wait is free for it).
inline int take_scratch(int dev, size_t bytes, Scratch *out, hipStream_t st)
{
    {
        std::lock_guard<std::mutex> lk(g_scratch_mu);
        for (size_t k = 0; k < g_scratch_free.size(); ++k) {
            Scratch &c = g_scratch_free[k];
            if (c.dev != dev || c.bytes < bytes) continue;
            if (c.busy && (c.busy_on != st || st == hipStreamPerThread)) {
                if (hipEventQuery(c.ev) != hipSuccess) {
                    (void)hipGetLastError();            // (hipErrorNotReady is no failure of this call)
                    continue;
                }
                c.busy = false;
            }
            *out = c;
            out->busy = false;
            g_scratch_free.erase(g_scratch_free.begin() + (long)k);
            return SS_OK;
        }
    }
    Scratch sc;
    sc.dev = dev;
    sc.bytes = (bytes + 4095) & ~(size_t)4095;
    HIP_TRY(hipMalloc(reinterpret_cast<void **>(&sc.d), sc.bytes));
    hipError_t e = hipHostMalloc(reinterpret_cast<void **>(&sc.h), sizeof(uint64_t), hipHostMallocDefault);
    if (e == hipSuccess) {
        e = hipEventCreateWithFlags(&sc.ev, hipEventDisableTiming);
        if (e != hipSuccess) (void)hipHostFree(sc.h);
    }
    if (e != hipSuccess) {
        (void)hipFree(sc.d);
        return fail(SS_ERR_HIP, "scratch of an all-matches call: %s", hipGetErrorString(e));
    }
    *out = sc;
    return SS_OK;
}

struct ScratchLease {
    Scratch sc;
    bool done = false;          // the call's stream wait has returned: nothing of it is still using the buffer
    // A call that does not wait: the buffer goes back behind everything enqueued on `st` so far.
    int release_on(hipStream_t st)
    {
        HIP_TRY(hipEventRecord(sc.ev, st));
        sc.busy = true;
        sc.busy_on = st;
        done = true;
        return SS_OK;
    }
    ~ScratchLease()
    {
        if (!done || !sc.d) return;
        std::lock_guard<std::mutex> lk(g_scratch_mu);
        g_scratch_free.push_back(sc);
    }
};

}  // namespace ssh
