// What the units behind the extern "C" boundary share (runtime.hip, host_pipe.hip, fir_api.hip, iir_api.hip, capi.hip).
// No kernel unit includes this header.
#pragma once
#include "skdsp_internal.hpp"
#include "stage_plan.hpp"
#include <algorithm>

namespace skdsp {

// every entry point that needs a device: bind slot 0 on first use, then hold the calling slot's lock for the call
#define API_BEGIN                        \
    {                                    \
        int _rc = ensure_init();         \
        if (_rc) return _rc;             \
    }                                    \
    std::lock_guard<std::mutex> _ctxlk(ctx().mu)

template <typename H> static H *as_handle(skdsp_handle h, int kind)
{
    HandleBase *b = reinterpret_cast<HandleBase *>(h);
    if (!b || b->kind != kind) return nullptr;
    return static_cast<H *>(b);
}

static inline size_t round_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// ---- runtime.hip ------------------------------------------------------------------------------------------------
int sync_checked();   // stream sync of the calling slot + the deferred failures of what ran on it

// ---- host_pipe.hip ----------------------------------------------------------------------------------------------
// the staging of a host-pointer call (stage_plan.hpp has the rules).  stage_begin: every workspace slot reserved once with its summed size, the
// host-to-device copies issued.  stage_finish: the device-to-host copies (float32 / complex64 results widened on the device for a wide_out
// handle), then the call's one sync_checked -- also with nothing to copy back.  launch_rc: what the launch between the two returned; a failure
// is handed back as it is
static_assert(kStageHeadroom == (size_t)kHeadroomBytes, "stage_plan.hpp keeps the primary input behind the same headroom");
int stage_begin(StagePlan &p);
int stage_finish(const StagePlan &p, int launch_rc, const HandleBase *h = nullptr);
void pipe_free(Context &c);   // the slot's chunk pipeline state (skdsp_shutdown)

// how a long vector is cut: chunk k covers inputs [k C, min((k+1) C, n)) and outputs [(k C L) / M, (end L) / M)
struct ChunkPlan {
    int64_t n = 0, C = 0, nchunks = 0, hist = 0;
    int L = 1, M = 1;
    size_t esz = 0;       // bytes per input / output sample on the device
    bool wide = false;    // results leave as float64 / complex128 (twice esz on the host side)
    int64_t in_begin(int64_t k) const { return k * C; }
    int64_t in_end(int64_t k) const { return std::min<int64_t>((k + 1) * C, n); }
    int64_t hist_of(int64_t k) const { return std::min<int64_t>(hist, k * C); }
    int64_t out_begin(int64_t k) const { return (in_begin(k) * L) / M; }
    int64_t out_end(int64_t k) const { return k + 1 == nchunks ? (n * L) / M : (in_end(k) * L) / M; }
};
ChunkPlan plan_chunks(int64_t n, int L, int M, int64_t hist, size_t esz, bool wide, int chunk_log2);

typedef int (*chunk_kernel_fn)(void *self, const void *x_dev, int64_t n_k, int64_t n_hist, void *y_dev, int64_t k);
// Deal the chunks of a plan to the bound slots (at most max_slots of them; 0: no limit) and run the pipeline on each
int run_on_slots(const ChunkPlan &p, const char *x, char *y, chunk_kernel_fn kern, void *(*make_self)(void *, int), void *base_self,
                 bool allow_multi, int max_slots = 0);

}  // namespace skdsp
