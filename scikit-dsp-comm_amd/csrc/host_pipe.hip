// host_pipe.hip -- host-pointer staging and the chunk pipeline of the host-pointer entry points (see include/skdsp.h).
#include "api_internal.hpp"
#include <cstdio>
#include <cstring>
#include <thread>
#include <condition_variable>

namespace skdsp {

// The staging of a host-pointer call (stage_plan.hpp): the primary input into workspace 0 behind the headroom, the further pieces into
// workspace 1, the scratch in workspace 3 -- each slot reserved once, before any pointer into it is used.
int stage_begin(StagePlan &p)
{
    SK_CHECK(!p.overflow, SKDSP_ERR_BADARG, "staging: more than %d pieces declared", StagePlan::kMaxPieces);
    int rc = SKDSP_OK;
    if (p.scratch_bytes && (rc = ws_reserve(3, p.scratch_bytes, &p.scratch))) return rc;
    if (!p.host) return SKDSP_OK;
    if ((rc = ws_reserve(0, p.total0(), &p.base0))) return rc;
    if (p.npiece && (rc = ws_reserve(1, p.total1(), &p.base1))) return rc;
    if (p.in_bytes) SK_HIP(hipMemcpyAsync(p.in_dev(), p.in, p.in_bytes, hipMemcpyHostToDevice, ctx().stream));
    for (int i = 0; i < p.npiece; ++i)
        if (p.piece[i].src && p.piece[i].bytes) SK_HIP(hipMemcpyAsync(p.dev(i), p.piece[i].src, p.piece[i].bytes, hipMemcpyHostToDevice, ctx().stream));
    return SKDSP_OK;
}

int stage_finish(const StagePlan &p, int launch_rc, const HandleBase *h)
{
    if (launch_rc || !p.host) return launch_rc;
    // a wide_out handle: widen on the device into workspace 0 (it held the input, which the kernels are done with in stream order), piece i at
    // twice its offset -- one reserve for all of them
    const bool widen = h && h->wide_out && !dtype_double(h->dtype);
    void *wide = nullptr;
    int rc = SKDSP_OK;
    if (widen && (rc = ws_reserve(0, 2 * p.total1(), &wide))) return rc;
    for (int i = 0; i < p.npiece; ++i) {
        const StagePlan::Piece &q = p.piece[i];
        if (!q.dst || !q.bytes) continue;
        const void *from = p.dev(i);
        if (widen) {
            if ((rc = widen_launch(from, (int64_t)(q.bytes / 4), (char *)wide + 2 * q.off, ctx().stream))) return rc;
            from = (char *)wide + 2 * q.off;
        }
        SK_HIP(hipMemcpyAsync(q.dst, from, widen ? 2 * q.bytes : q.bytes, hipMemcpyDeviceToHost, ctx().stream));
    }
    return sync_checked();
}

// ---------------------------------------------------------------------------------------------------------------
// Host-pointer entry points on LONG vectors: chunk pipeline.
//
// The reference call hands over a NumPy array and expects one back (multirate_helper.py:104-127, 169-192), so the
// drop-in path crosses PCIe twice: 2 x 2.4 ms per 128 MiB against 0.06 ms of kernel.  Staging the whole vector,
// filtering it and copying it back one after the other leaves each PCIe direction idle half of the time.  Here the
// vector is cut into chunks of 2^host_chunk_log2 samples that are exact continuations of each other (FIR: the chunk's
// copy starts Ntaps-1 samples early and the kernel gets them as n_hist; IIR: zi / zf), and three things run at once:
//   the caller's thread   H2D of chunk k+1 (pageable source: the runtime's own staging runs at the link rate) and the
//                         launches of chunk k (compute stream waits for the copy's event)
//   a helper thread       D2H of chunk k-1 into the caller's result array (the other direction of the link)
// with two device buffers per direction.  With several slots bound (skdsp_init_devices: one per GPU) the chunks of a FIR
// are dealt to all of them -- each slot runs this pipeline over a contiguous range of chunks from its own worker thread
// and over its own PCIe link; the history of a range's first chunk comes from the host vector like any other chunk's,
// so the GPUs exchange nothing.
struct HostPipe {
    hipStream_t s_in = nullptr, s_out = nullptr;
    hipEvent_t in_ready[2] = {nullptr, nullptr}, done[2] = {nullptr, nullptr};
    void *din[2] = {nullptr, nullptr}, *dout[2] = {nullptr, nullptr};
    size_t cap_in = 0, cap_out = 0;
};

void pipe_free(Context &c)
{
    HostPipe *p = c.pipe;
    if (!p) return;
    for (int i = 0; i < 2; ++i) {
        if (p->din[i]) (void)hipFree(p->din[i]);
        if (p->dout[i]) (void)hipFree(p->dout[i]);
        if (p->in_ready[i]) (void)hipEventDestroy(p->in_ready[i]);
        if (p->done[i]) (void)hipEventDestroy(p->done[i]);
    }
    if (p->s_in) (void)hipStreamDestroy(p->s_in);
    if (p->s_out) (void)hipStreamDestroy(p->s_out);
    delete p;
    c.pipe = nullptr;
}

static int pipe_ensure(Context &c, size_t in_bytes, size_t out_bytes)
{
    if (!c.pipe) {
        HostPipe *p = new HostPipe();
        c.pipe = p;
        SK_HIP(hipStreamCreateWithFlags(&p->s_in, hipStreamNonBlocking));
        SK_HIP(hipStreamCreateWithFlags(&p->s_out, hipStreamNonBlocking));
        for (int i = 0; i < 2; ++i) {
            SK_HIP(hipEventCreateWithFlags(&p->in_ready[i], hipEventDisableTiming));
            SK_HIP(hipEventCreateWithFlags(&p->done[i], hipEventDisableTiming));
        }
    }
    HostPipe *p = c.pipe;
    if (in_bytes > p->cap_in) {
        SK_HIP(hipStreamSynchronize(c.stream));
        for (int i = 0; i < 2; ++i) {
            if (p->din[i]) SK_HIP(hipFree(p->din[i]));
            p->din[i] = nullptr;
        }
        p->cap_in = 0;
        for (int i = 0; i < 2; ++i) SK_HIP(hipMalloc(&p->din[i], in_bytes));
        p->cap_in = in_bytes;
    }
    if (out_bytes > p->cap_out) {
        SK_HIP(hipStreamSynchronize(c.stream));
        for (int i = 0; i < 2; ++i) {
            if (p->dout[i]) SK_HIP(hipFree(p->dout[i]));
            p->dout[i] = nullptr;
        }
        p->cap_out = 0;
        for (int i = 0; i < 2; ++i) SK_HIP(hipMalloc(&p->dout[i], out_bytes));
        p->cap_out = out_bytes;
    }
    return SKDSP_OK;
}

// the planner (also exported for the CPU tests: skdsp_host_chunk_plan)
ChunkPlan plan_chunks(int64_t n, int L, int M, int64_t hist, size_t esz, bool wide, int chunk_log2)
{
    ChunkPlan p;
    p.n = n; p.L = L; p.M = M; p.hist = hist; p.esz = esz; p.wide = wide;
    int64_t C = (int64_t)1 << std::max(10, std::min(chunk_log2, 30));
    C = std::max<int64_t>(C / M, 1) * M;       // chunk starts stay multiples of M: output phase 0 stays aligned
    if (C < hist) C = ((hist + M - 1) / M) * M;  // (keeps the staging buffers within twice a chunk)
    p.C = C;
    p.nchunks = std::max<int64_t>((n + C - 1) / C, 1);
    return p;
}

// chunks [k0, k1) of the plan on the CURRENT slot; x / y: the caller's whole host vectors
static int run_pipeline(const ChunkPlan &p, int64_t k0, int64_t k1, const char *x, char *y, chunk_kernel_fn kern, void *self)
{
    Context &c = ctx();
    if (k1 <= k0) return SKDSP_OK;
    const size_t esz = p.esz, esz_out = p.wide ? 2 * esz : esz;
    const size_t in_cap = (size_t)(p.C + p.hist) * esz + kHeadroomBytes + 512;
    const size_t out_cap = (size_t)((p.C * p.L) / p.M + 2) * esz_out + 512;
    int rc = pipe_ensure(c, in_cap, out_cap);
    if (rc) return rc;
    HostPipe *hp = c.pipe;
    void *narrow = nullptr;
    if (p.wide && (rc = ws_reserve(1, (size_t)((p.C * p.L) / p.M + 2) * esz + 256, &narrow))) return rc;

    std::mutex mu;
    std::condition_variable cv;
    int64_t posted = k0, drained = k0;   // chunks handed to / finished by the copy-back thread
    bool abort_flag = false;
    int helper_rc = SKDSP_OK;
    char helper_err[256] = "";
    const int device = c.device;
    std::thread helper([&]() {
        if (hipSetDevice(device) != hipSuccess) {
            std::lock_guard<std::mutex> lk(mu);
            helper_rc = SKDSP_ERR_HIP;
            snprintf(helper_err, sizeof(helper_err), "host pipeline: hipSetDevice(%d) failed in the copy-back thread", device);
            drained = k1;
            cv.notify_all();
            return;
        }
        for (int64_t k = k0; k < k1; ++k) {
            {
                std::unique_lock<std::mutex> lk(mu);
                cv.wait(lk, [&] { return posted > k || abort_flag; });
                if (abort_flag && posted <= k) break;
            }
            const int b = (int)((k - k0) & 1);
            const size_t bytes = (size_t)(p.out_end(k) - p.out_begin(k)) * esz_out;
            hipError_t e = hipEventSynchronize(hp->done[b]);
            if (e == hipSuccess && bytes)
                e = hipMemcpyAsync(y + (size_t)p.out_begin(k) * esz_out, hp->dout[b], bytes, hipMemcpyDeviceToHost, hp->s_out);
            if (e == hipSuccess) e = hipStreamSynchronize(hp->s_out);
            std::lock_guard<std::mutex> lk(mu);
            if (e != hipSuccess && helper_rc == SKDSP_OK) {
                helper_rc = SKDSP_ERR_HIP;
                snprintf(helper_err, sizeof(helper_err), "host pipeline: copy back of chunk %lld failed: %s", (long long)k, hipGetErrorString(e));
            }
            drained = k + 1;
            cv.notify_all();
        }
        std::lock_guard<std::mutex> lk(mu);
        drained = k1;
        cv.notify_all();
    });

    auto body = [&]() -> int {
        for (int64_t k = k0; k < k1; ++k) {
            const int b = (int)((k - k0) & 1);
            const int64_t hk = p.hist_of(k), ib = p.in_begin(k), nk = p.in_end(k) - ib;
            // din[b] was last read by the kernels of chunk k-2; dout[b] was last read by the copy back of chunk k-2
            if (k - k0 >= 2) {
                SK_HIP(hipEventSynchronize(hp->done[b]));
                std::unique_lock<std::mutex> lk(mu);
                cv.wait(lk, [&] { return drained >= k - 1 || helper_rc != SKDSP_OK; });
                if (helper_rc != SKDSP_OK) return helper_rc;
            }
            char *xd = (char *)hp->din[b] + kHeadroomBytes + (size_t)p.hist * esz;
            xd = (char *)(((uintptr_t)xd + 255) & ~(uintptr_t)255);   // x[0] of the chunk 256-byte aligned, history in front of it
            SK_HIP(hipMemcpyAsync(xd - (size_t)hk * esz, x + (size_t)(ib - hk) * esz, (size_t)(nk + hk) * esz, hipMemcpyHostToDevice, hp->s_in));
            SK_HIP(hipEventRecord(hp->in_ready[b], hp->s_in));
            SK_HIP(hipStreamWaitEvent(c.stream, hp->in_ready[b], 0));
            const int64_t n_out = p.out_end(k) - p.out_begin(k);
            void *yd = p.wide ? narrow : hp->dout[b];
            int r = kern(self, xd, nk, hk, yd, k);
            if (r) return r;
            if (p.wide && n_out > 0 && (r = widen_launch(narrow, (int64_t)((size_t)n_out * esz / 4), hp->dout[b], c.stream))) return r;
            SK_HIP(hipEventRecord(hp->done[b], c.stream));
            {
                std::lock_guard<std::mutex> lk(mu);
                posted = k + 1;
            }
            cv.notify_all();
        }
        return SKDSP_OK;
    };
    rc = body();
    {
        std::lock_guard<std::mutex> lk(mu);
        if (rc) abort_flag = true;
    }
    cv.notify_all();
    helper.join();
    (void)hipStreamSynchronize(c.stream);
    if (rc) return rc;
    if (helper_rc) {
        set_error("%s", helper_err);
        return helper_rc;
    }
    return async_err_check(c);
}

// Deal the chunks of a plan to every bound slot (contiguous ranges); make_self(slot) gives the per-slot kernel argument
// (the handle's clone on that slot).  One worker thread per extra slot; the caller's thread serves its own slot.
// max_slots > 0: this call uses at most that many slots (skdsp_fir_filter_sharded)
int run_on_slots(const ChunkPlan &p, const char *x, char *y, chunk_kernel_fn kern, void *(*make_self)(void *, int), void *base_self,
                 bool allow_multi, int max_slots)
{
    const int home = ctx().slot;
    int nslots = allow_multi && opt().host_multi_slot ? slot_count() : 1;
    if (max_slots > 0 && nslots > max_slots) nslots = max_slots;
    if (nslots > p.nchunks) nslots = (int)p.nchunks;
    if (nslots <= 1) return run_pipeline(p, 0, p.nchunks, x, y, kern, make_self(base_self, home));
    std::vector<void *> selfs((size_t)nslots, nullptr);
    std::vector<int> slots;
    slots.push_back(home);
    for (int s = 0; s < slot_count() && (int)slots.size() < nslots; ++s)
        if (s != home && ctx_of(s).ready) slots.push_back(s);
    nslots = (int)slots.size();
    for (int i = 0; i < nslots; ++i) {
        selfs[i] = make_self(base_self, slots[i]);
        if (!selfs[i]) return SKDSP_ERR_NOMEM;
    }
    std::vector<int> rcs((size_t)nslots, SKDSP_OK);
    std::vector<std::string> errs((size_t)nslots), paths((size_t)nslots);   // (paths: the engines each worker thread launched -- the record is thread-local)
    std::vector<std::thread> workers;
    auto range = [&](int i, int64_t &a, int64_t &b) {
        a = p.nchunks * i / nslots;
        b = p.nchunks * (i + 1) / nslots;
    };
    for (int i = 1; i < nslots; ++i) {
        workers.emplace_back([&, i]() {
            int r = select_slot(slots[i]);
            if (!r) {
                std::lock_guard<std::mutex> lk(ctx().mu);   // the slot's own lock: other callers' workers wait here
                int64_t a, b;
                range(i, a, b);
                r = run_pipeline(p, a, b, x, y, kern, selfs[i]);
            }
            rcs[i] = r;
            if (r) errs[i] = skdsp_last_error();
            char pb[256];
            skdsp_debug_path(pb, (int)sizeof(pb), 1);
            paths[i] = pb;
        });
    }
    {
        int64_t a, b;
        range(0, a, b);
        rcs[0] = run_pipeline(p, a, b, x, y, kern, selfs[0]);
    }
    for (auto &w : workers) w.join();
    for (int i = 1; i < nslots; ++i) {   // what the workers launched belongs to the caller's record: engine by engine, through the same de-duplication
        size_t at = 0;
        while (at < paths[i].size()) {
            size_t e = paths[i].find(',', at);
            if (e == std::string::npos) e = paths[i].size();
            if (e > at) note_path(paths[i].substr(at, e - at).c_str());
            at = e + 1;
        }
    }
    for (int i = 0; i < nslots; ++i)
        if (rcs[i]) {
            if (i > 0) set_error("%s", errs[i].c_str());
            return rcs[i];
        }
    return SKDSP_OK;
}

}  // namespace skdsp

using namespace skdsp;

extern "C" {

// the chunk planner of the host pipeline, exported for tests: chunk k of (n, L, M, hist) -> input / output ranges
int skdsp_host_chunk_plan(int64_t n, int L, int M, int64_t hist, int chunk_log2, int64_t k, int64_t *nchunks, int64_t *in_begin,
                          int64_t *in_end, int64_t *in_hist, int64_t *out_begin, int64_t *out_end)
{
    SK_CHECK(n >= 0 && L >= 1 && M >= 1 && hist >= 0, SKDSP_ERR_BADARG, "host_chunk_plan: bad arguments");
    const ChunkPlan p = plan_chunks(n, L, M, hist, 1, false, chunk_log2);
    if (nchunks) *nchunks = p.nchunks;
    SK_CHECK(k >= 0 && k < p.nchunks, SKDSP_ERR_BADARG, "host_chunk_plan: chunk %lld of %lld", (long long)k, (long long)p.nchunks);
    if (in_begin) *in_begin = p.in_begin(k);
    if (in_end) *in_end = p.in_end(k);
    if (in_hist) *in_hist = p.hist_of(k);
    if (out_begin) *out_begin = p.out_begin(k);
    if (out_end) *out_end = p.out_end(k);
    return SKDSP_OK;
}

}  // extern "C"
