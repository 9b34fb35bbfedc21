// fir_api.hip -- FIR execution behind the extern "C" boundary (see include/skdsp.h): fir_run launches what fir_route (fir_route.hpp: the
// applicability rules, the measured cost models, tap segments, heads) decided for the call; the handles of tap segments and heads; rows; the
// FIR entry points.
#include "api_internal.hpp"
#include "fir_route.hpp"

namespace skdsp {

static_assert(kFirF32 == SKDSP_F32 && kFirC64 == SKDSP_C64 && kFirF64 == SKDSP_F64 && kFirC128 == SKDSP_C128, "fir_route.hpp restates the dtype codes");
static_assert(kFirAuto == SKDSP_FIR_AUTO && kFirDirect == SKDSP_FIR_DIRECT && kFirOls == SKDSP_FIR_OLS, "fir_route.hpp restates the algorithm codes");

// the options the router reads
static FirRouteOptions fir_route_options()
{
    const Options &o = opt();
    FirRouteOptions r;
    r.fir_algo = o.fir_algo; r.dn_no_ols = o.dn_no_ols; r.fir_mm = o.fir_mm; r.fir_bx = o.fir_bx;
    r.fir_up_ols_min = o.fir_up_ols_min; r.fir_up_rows_min = o.fir_up_rows_min; r.fir_up_pair = o.fir_up_pair;
    r.fir_up4k = o.fir_up4k; r.fir_up2k = o.fir_up2k; r.fir_up_rep = o.fir_up_rep;
    r.fir_dn_fold = o.fir_dn_fold; r.fir_dn4k = o.fir_dn4k; r.fir_updn_fused = o.fir_updn_fused;
    return r;
}

int fir_algo_for(const FirHandle *h, int64_t n) { return pick_fir_algo(fir_shape_of(h), n, fir_route_options()); }

// the handles of tap segments and heads are made below; the device memory of a handle frees itself (dev_mem.hpp)
FirHandle::~FirHandle()
{
    for (FirHandle *p : parts) delete p;
    for (FirHandle *p : heads) delete p;
}

// ---- tap partitioning: filters longer than one launch takes ------------------------------------------------------
// The reference accepts any tap count (lfilter(b,[1],x), multirate_helper.py:108).  One launch takes up to 4097 taps in
// the overlap-save engine (float32 / complex64) and a few thousand in the float64 direct-form kernels (LDS window); a
// longer b is cut into segments of `seg` taps,  y[m] = sum_s (b_s * x)[m - s seg]:  segment s is an ordinary filter
// launch over the input shortened by its delay (with as much of the caller's history as it can still see), and its
// result is added onto y from output s seg on.  For .dn the segment length is a multiple of M, so every partial
// result keeps decimation phase 0.
// A handle over taps [t0, t0 + cnt) of `h` on slot `slot`: the ONE place that copies a FIR handle's fields (tap segments, the heads of short calls,
// the per-slot clones of the multi-GPU host path), so that a field added to FirHandle cannot be forgotten in one of them.
static FirHandle *fir_derive(const FirHandle *h, int t0, int cnt, int slot)
{
    const int comp = h->taps_complex ? 2 : 1;
    FirHandle *d = new FirHandle();
    d->kind = H_FIR; d->dtype = h->dtype; d->slot = slot; d->taps_complex = h->taps_complex; d->algo = h->algo; d->wide_out = h->wide_out;
    d->ntaps = cnt;
    d->taps_host.assign(h->taps_host.begin() + (size_t)t0 * comp, h->taps_host.begin() + (size_t)(t0 + cnt) * comp);
    return d;
}

static int fir_run(FirHandle *h, const FirRoute &r, const void *x_dev, int64_t n, int64_t n_hist, void *y_dev);

// y[j] = L sum_t b[(j M mod L) + L t] x[(j M div L) - t] with b cut into segments of `seg` taps, seg a multiple of lcm(L, M):
// segment s delays the up-rate signal by s seg samples = s seg / L input samples = s seg / M outputs, so it is the same
// operation over the input shortened by s seg / L samples, added onto y from output s seg / M on.  With history in front
// of x the segment starts d input samples early (d a multiple of M / gcd(L, M): whole outputs) and lands d L / M outputs earlier
// (the lengths: fir_parts_seg, fir_parts_segment, fir_parts_history_ok in fir_route.hpp).
static int fir_parts_run(FirHandle *h, int seg, const void *x_dev, int64_t n, int64_t n_hist, int L, int M, void *y_dev)
{
    const FirShape shape = fir_shape_of(h);
    SK_CHECK(fir_parts_seg_ok(shape, seg, L), SKDSP_ERR_UNSUPPORTED, "fir: %d taps with L/M = %d/%d: one output period (%d taps) is longer than a launch takes", h->ntaps, L, M, seg);
    if (h->part_seg != seg) {
        for (FirHandle *p : h->parts) delete p;
        h->parts.clear();
        for (int t0 = 0; t0 < h->ntaps; t0 += seg) h->parts.push_back(fir_derive(h, t0, std::min(seg, h->ntaps - t0), h->slot));
        h->part_seg = seg;
    }
    for (FirHandle *p : h->parts) p->algo = h->algo;   // (skdsp_fir_set_algo after the parts were made)
    SK_CHECK(fir_parts_history_ok(shape, seg, L, M, n_hist), SKDSP_ERR_UNSUPPORTED,
             "fir: %d taps run as %d tap segments; with L/M = %d/%d a partial history (n_hist = %lld < %lld) must be a multiple of %d samples",
             h->ntaps, (int)h->parts.size(), L, M, (long long)n_hist, (long long)((int64_t)(h->parts.size() - 1) * seg / L), M / std::gcd(L, M));
    const size_t esz = dtype_size(h->dtype);
    const int scal = dtype_complex(h->dtype) ? 2 : 1;
    const FirRouteOptions o = fir_route_options();
    void *tmp = nullptr;
    int rc = ws_reserve(2, (size_t)((n * L) / M + 1) * esz + 256, &tmp);
    if (rc) return rc;
    for (size_t si = 0; si < h->parts.size(); ++si) {
        FirHandle *p = h->parts[si];
        FirSegment sg;
        if (!fir_parts_segment(shape, seg, (int)si, n, n_hist, L, M, &sg)) break;
        const char *xs = (const char *)x_dev - (size_t)sg.d * esz;
        void *dst = si == 0 ? y_dev : tmp;
        // (workspace slot 2 is `tmp` -- possibly `dst` -- here: scratch_free = false, no scratch-using forms; a segment writes (n_s L) / M <= n_out outputs)
        const FirCall c{sg.n, sg.n_hist, L, M, L == 1 && M == 1, (unsigned)(uintptr_t)dst, false, ctx().num_cus};
        if ((rc = fir_run(p, fir_route_single(fir_shape_of(p), c, o), xs, sg.n, sg.n_hist, dst))) return rc;
        if (si > 0 && (rc = accumulate_launch((char *)y_dev + (size_t)sg.off * esz, tmp, sg.cnt * scal, dtype_double(h->dtype), ctx().stream))) return rc;
    }
    return SKDSP_OK;
}

// A call from rest over n < Ntaps samples computes y[m] = sum_(k <= m) b[k] x[m - k], m < n: taps b[n ...] are never reached.  It runs on a
// copy of the filter cut to the next power of two >= n (at most log2(Ntaps) copies per handle) -- the same outputs exactly, less work, and
// the rounding of a float32 engine (a few 1e-8 of sum |b| max |x|: the FFT engines round against the WHOLE filter) shrinks with the taps
// that matter.  (Found by the differential test at north_star's bound without its former factor 2: 17 rows of 100 samples through a
// 1024-tap low-pass, whose first 100 taps are its tail -- 1.7e-6 of the tiny start-up transient before, far inside 1e-6 after.)
static FirHandle *fir_head(FirHandle *h, int64_t n)
{
    const int keep = fir_head_taps(h->ntaps, n);
    if (!keep) return h;
    for (FirHandle *t : h->heads)
        if (t->ntaps == keep) { t->algo = h->algo; return t; }
    // (at most log2(Ntaps) <= 13 heads per handle -- one per power of two below the tap count -- each with the tables of the engines it has run on: they
    // live as long as the handle)
    FirHandle *t = fir_derive(h, 0, keep, h->slot);
    h->heads.push_back(t);
    return t;
}

// Launch what the router decided.  Workspace: slot 2 holds the sums of a tap-segment call, the rows of the .up walk, the unfused L / M copy or the
// full-rate result of .dn's last resort (slot 3 inside a tap-segment call -- the planes of a complex IIR call, never alive during a FIR call).
static int fir_run(FirHandle *h, const FirRoute &r, const void *x_dev, int64_t n, int64_t n_hist, void *y_dev)
{
    hipStream_t s = ctx().stream;
    const int L = r.L, M = r.M;
    if (r.direct_refused) note_path("fir_direct");   // (the polyphase launcher, which has no kernel for this stride, stays the first name of the path)
    if (r.copy == kCopyFullRate) {   // the last resort of .dn: the full-rate filter, and a strided copy
        void *full = nullptr;
        const int64_t nk = (n / M) * M;
        int rc = ws_reserve(r.slot, (size_t)nk * dtype_size(h->dtype) + 256, &full);
        if (rc) return rc;
        FirRoute f = r;
        f.M = 1; f.copy = kCopyNone; f.direct_refused = false;
        if ((rc = fir_run(h, f, x_dev, nk, n_hist, full))) return rc;
        return downsample_launch(full, nk, M, 0, h->dtype, y_dev, s);
    }
    if (r.head) h = fir_head(h, n);
    const bool dbl = dtype_double(h->dtype);
    auto walk = [&](void *out, int dec, int64_t pitch, int paired) {
        return dbl ? fir_ols64_up_launch(h, x_dev, n, n_hist, L, out, s, dec, pitch, paired) : fir_ols_up_launch(h, x_dev, n, n_hist, L, out, s, dec, pitch, paired);
    };
    switch (r.engine) {
    case kRouteNone: return SKDSP_OK;
    case kRouteParts: return fir_parts_run(h, r.seg, x_dev, L == 1 ? (n / M) * M : n, n_hist, L, M, y_dev);
    case kRouteRefused:   // (whoever refuses says why: the history rule of the tap segments, or the polyphase launcher)
        if (r.seg) return fir_parts_run(h, r.seg, x_dev, L == 1 ? (n / M) * M : n, n_hist, L, M, y_dev);
        return fir_direct_launch(h, kRouteDirect, x_dev, n, n_hist, L, M, (n * L) / M, y_dev, s);
    case kRouteBx: case kRouteMm: case kRouteDirect: return fir_direct_launch(h, r.engine, x_dev, n, n_hist, L, M, (n * L) / M, y_dev, s);
    case kRouteOls: return fir_ols_launch(h, x_dev, n, n_hist, y_dev, s, r.dec);
    case kRouteOls64: return fir_ols64_launch(h, x_dev, n, n_hist, y_dev, s, r.dec);
    case kRouteDn4k: return fir_dn4k_launch(h, x_dev, n, n_hist, M, y_dev, s);
    case kRouteUp4k: return fir_up4k_launch(h, x_dev, n, n_hist, L, y_dev, s);
    case kRouteUp2k: return fir_up2k_launch(h, x_dev, n, n_hist, L, y_dev, s);
    case kRouteOlsRep: return fir_ols_rep_launch(h, x_dev, n, n_hist, L, y_dev, s);
    case kRouteWalk: case kRouteWalk64: break;
    default: SK_CHECK(false, SKDSP_ERR_BADARG, "fir: bad route %d", r.engine);
    }
    if (r.copy == kCopyWeave) {   // the phases leave as rows with the plain filter's stores, and interleave_launch weaves them
        const int rows_n = r.paired ? L / 2 : L;
        const int row_dtype = r.paired ? (dbl ? SKDSP_C128 : SKDSP_C64) : h->dtype;
        const int64_t pitch = (int64_t)round_up((size_t)n, 64);
        void *rows = nullptr;
        int rc = ws_reserve(r.slot, (size_t)pitch * rows_n * dtype_size(row_dtype) + 256, &rows);
        if (rc) return rc;
        if ((rc = walk(rows, 1, pitch, r.paired))) return rc;
        return interleave_launch(rows, n, rows_n, pitch, row_dtype, y_dev, s);
    }
    if (r.copy == kCopyEveryMth) {   // all n L outputs to scratch, every M-th of them kept
        void *full = nullptr;
        int rc = ws_reserve(r.slot, (size_t)n * L * dtype_size(h->dtype) + 256, &full);
        if (rc) return rc;
        if ((rc = walk(full, 1, 0, 0))) return rc;
        return downsample_launch(full, n * L, M, 0, h->dtype, y_dev, s);
    }
    return walk(y_dev, r.dec, 0, r.paired);
}

// one call of an entry point: fill FirCall, route, run (L = M = 1 with plain = false: the rate changers' entry points at rate 1)
static int fir_call(FirHandle *h, const void *x_dev, int64_t n, int64_t n_hist, int L, int M, bool plain, void *y_dev)
{
    const FirCall c{n, n_hist, L, M, plain, (unsigned)(uintptr_t)y_dev, true, ctx().num_cus};
    return fir_run(h, fir_route(fir_shape_of(h), c, fir_route_options()), x_dev, n, n_hist, y_dev);
}
static int fir_filter_any(FirHandle *h, const void *x_dev, int64_t n, int64_t n_hist, void *y_dev) { return fir_call(h, x_dev, n, n_hist, 1, 1, true, y_dev); }
static int fir_dn_any(FirHandle *h, const void *x_dev, int64_t n, int64_t n_hist, int M, void *y_dev) { return fir_call(h, x_dev, n, n_hist, 1, M, false, y_dev); }
static int fir_updn_any(FirHandle *h, const void *x_dev, int64_t n, int64_t n_hist, int L, int M, void *y_dev) { return fir_call(h, x_dev, n, n_hist, L, M, false, y_dev); }

}  // namespace skdsp

using namespace skdsp;

extern "C" {

// ------------------------------------------------------------------------ FIR
int skdsp_fir_create(const void *taps, int ntaps, int taps_complex, int dtype, skdsp_handle *out)
{
    API_BEGIN;
    SK_CHECK(out, SKDSP_ERR_BADARG, "fir_create: null out");
    SK_CHECK(taps && ntaps >= 1, SKDSP_ERR_BADARG, "fir_create: need at least one tap");
    SK_CHECK(dtype_valid(dtype), SKDSP_ERR_BADARG, "fir_create: bad dtype %d", dtype);
    SK_CHECK(!(taps_complex && !dtype_complex(dtype)), SKDSP_ERR_BADARG,
             "fir_create: complex taps need a complex signal dtype");
    std::unique_ptr<FirHandle> h(new FirHandle());
    h->kind = H_FIR;
    h->dtype = dtype;
    h->ntaps = ntaps;
    h->taps_complex = taps_complex != 0;
    const int comp = taps_complex ? 2 : 1;
    h->taps_host.assign((const double *)taps, (const double *)taps + (size_t)ntaps * comp);
    *out = h.release();
    return SKDSP_OK;
}

int skdsp_fir_set_algo(skdsp_handle hh, int algo)
{
    FirHandle *h = as_handle<FirHandle>(hh, H_FIR);
    SK_CHECK(h, SKDSP_ERR_BADARG, "fir_set_algo: not a FIR handle");
    SK_CHECK(algo >= SKDSP_FIR_AUTO && algo <= SKDSP_FIR_OLS, SKDSP_ERR_BADARG, "fir_set_algo: bad algo %d", algo);
    h->algo = algo;
    return SKDSP_OK;
}

int skdsp_fir_get_algo(skdsp_handle hh, int64_t n, int *algo_used)
{
    FirHandle *h = as_handle<FirHandle>(hh, H_FIR);
    SK_CHECK(h && algo_used, SKDSP_ERR_BADARG, "fir_get_algo: bad arguments");
    *algo_used = fir_algo_for(h, n);
    return SKDSP_OK;
}

int skdsp_fir_filter_dev(skdsp_handle hh, const void *x_dev, int64_t n, int64_t n_hist, void *y_dev)
{
    API_BEGIN;
    FirHandle *h = as_handle<FirHandle>(hh, H_FIR);
    SK_CHECK(h, SKDSP_ERR_BADARG, "fir_filter: not a FIR handle");
    SK_CHECK(n >= 0 && n_hist >= 0, SKDSP_ERR_BADARG, "fir_filter: negative length");
    std::lock_guard<std::mutex> lk(h->mu);
    return fir_filter_any(h, x_dev, n, n_hist, y_dev);
}

int skdsp_fir_up_dev(skdsp_handle hh, const void *x_dev, int64_t n, int64_t n_hist, int L, void *y_dev)
{
    API_BEGIN;
    FirHandle *h = as_handle<FirHandle>(hh, H_FIR);
    SK_CHECK(h, SKDSP_ERR_BADARG, "fir_up: not a FIR handle");
    SK_CHECK(L >= 1, SKDSP_ERR_BADARG, "fir_up: L must be >= 1");
    std::lock_guard<std::mutex> lk(h->mu);
    return fir_updn_any(h, x_dev, n, n_hist, L, 1, y_dev);
}

int skdsp_fir_dn_dev(skdsp_handle hh, const void *x_dev, int64_t n, int64_t n_hist, int M, void *y_dev)
{
    API_BEGIN;
    FirHandle *h = as_handle<FirHandle>(hh, H_FIR);
    SK_CHECK(h, SKDSP_ERR_BADARG, "fir_dn: not a FIR handle");
    SK_CHECK(M >= 1, SKDSP_ERR_BADARG, "fir_dn: M must be >= 1");
    std::lock_guard<std::mutex> lk(h->mu);
    return fir_dn_any(h, x_dev, n, n_hist, M, y_dev);
}

int skdsp_fir_updn_dev(skdsp_handle hh, const void *x_dev, int64_t n, int64_t n_hist, int L, int M, void *y_dev)
{
    API_BEGIN;
    FirHandle *h = as_handle<FirHandle>(hh, H_FIR);
    SK_CHECK(h, SKDSP_ERR_BADARG, "fir_updn: not a FIR handle");
    SK_CHECK(L >= 1 && M >= 1, SKDSP_ERR_BADARG, "fir_updn: L, M must be >= 1");
    std::lock_guard<std::mutex> lk(h->mu);
    return fir_updn_any(h, x_dev, n, n_hist, L, M, y_dev);
}

// one chunk of a long host vector (run_pipeline): the same launch as the single-shot path, with the chunk's history
struct FirChunkJob {
    FirHandle *h;
    int mode, L, M;
};
static int fir_chunk_kernel(void *self, const void *x_dev, int64_t n_k, int64_t n_hist, void *y_dev, int64_t)
{
    const FirChunkJob *j = static_cast<const FirChunkJob *>(self);
    if (j->mode == 0) return fir_filter_any(j->h, x_dev, n_k, n_hist, y_dev);
    if (j->L == 1) return fir_dn_any(j->h, x_dev, n_k, n_hist, j->M, y_dev);
    return fir_updn_any(j->h, x_dev, n_k, n_hist, j->L, j->M, y_dev);
}
// the job on another slot: same filter, tables on that slot's device (clone made once, owned by the handle)
struct FirChunkJobs {
    FirChunkJob home;                 // the caller's handle
    FirChunkJob other[kMaxSlots];     // its clones, filled as slots ask for them
};
static void *fir_job_on_slot(void *base, int slot)
{
    FirChunkJobs *js = static_cast<FirChunkJobs *>(base);
    FirHandle *h = js->home.h;
    if (slot == h->slot) return &js->home;
    if ((int)h->clones.size() < kMaxSlots) h->clones.resize(kMaxSlots, nullptr);
    if (!h->clones[slot]) {
        h->clones[slot] = fir_derive(h, 0, h->ntaps, slot);
    }
    js->other[slot] = FirChunkJob{static_cast<FirHandle *>(h->clones[slot]), js->home.mode, js->home.L, js->home.M};
    return &js->other[slot];
}

static int fir_host_call(skdsp_handle hh, const void *x, int64_t n, int L, int M, int mode, void *y, int max_slots = 0)
{
    API_BEGIN;
    FirHandle *h = as_handle<FirHandle>(hh, H_FIR);
    SK_CHECK(h, SKDSP_ERR_BADARG, "fir: not a FIR handle");
    SK_CHECK(n >= 0 && L >= 1 && M >= 1, SKDSP_ERR_BADARG, "fir: bad arguments (n=%lld L=%d M=%d)", (long long)n, L, M);
    const size_t esz = dtype_size(h->dtype);
    const int64_t n_out = mode == 0 ? n : (n * L) / M;
    if (n_out == 0) return SKDSP_OK;
    SK_CHECK(x && y, SKDSP_ERR_BADARG, "fir: null buffer");
    std::lock_guard<std::mutex> lk(h->mu);
    if (opt().host_pipeline && n > (((int64_t)3 << opt().host_chunk_log2) >> 1)) {
        // long vector: chunk pipeline (and every bound slot); exact by construction (n_hist)
        const int64_t hist = L > 1 ? (h->ntaps - 1 + L - 1) / L : h->ntaps - 1;
        const ChunkPlan p = plan_chunks(n, mode == 0 ? 1 : L, mode == 0 ? 1 : M, hist, esz, h->wide_out && !dtype_double(h->dtype),
                                        opt().host_chunk_log2);
        FirChunkJobs jobs;
        jobs.home = FirChunkJob{h, mode, L, M};
        return run_on_slots(p, (const char *)x, (char *)y, fir_chunk_kernel, fir_job_on_slot, &jobs, true, max_slots);
    }
    StagePlan p;
    p.input(x, (size_t)n * esz);
    const int iy = p.add_out(y, (size_t)n_out * esz);
    int rc = stage_begin(p);
    if (rc) return rc;
    if (mode == 0) rc = fir_filter_any(h, p.in_dev(), n, 0, p.dev(iy));
    else if (L == 1) rc = fir_dn_any(h, p.in_dev(), n, 0, M, p.dev(iy));
    else rc = fir_updn_any(h, p.in_dev(), n, 0, L, M, p.dev(iy));
    return stage_finish(p, rc, h);
}

// ---- N-D inputs: rows of one launch ---------------------------------------------------------------------------------
// lfilter(b, [1], x) filters along the last axis of an N-D array in one call (multirate_helper.py:108).  A FIR forgets
// after Ntaps-1 samples, so the rows are laid end to end with Ntaps-1 zeros between them and filtered as ONE signal from
// rest: every output sees exactly the window a launch over its row alone would see (zeros in front of every row), so the
// results agree to the kernels' rounding (the overlap-save tile boundaries fall elsewhere).  Host form: one pitched copy in, one launch, one pitched copy out;
// device form: the two pitched copies are device-to-device.  Costs (Ntaps-1)/n extra samples.
constexpr size_t kRowsBlockBudget = (size_t)16 << 30;   // bytes of the staged block of an N-D call (its output block is as large again)
static int64_t fir_rows_pitch(FirHandle *h, int64_t n) { return (int64_t)round_up((size_t)(n + fir_head(h, n)->ntaps - 1), 4); }

static int fir_rows_run(FirHandle *h, int64_t n, int64_t nrow, int64_t pitch, void *xp, void *yp)
{
    h = fir_head(h, n);   // (rows shorter than the filter: only the first n taps are ever reached)
    const size_t esz = dtype_size(h->dtype);
    // zeros between the rows (the last row needs none behind it)
    if (nrow > 1)
        SK_HIP(hipMemset2DAsync((char *)xp + (size_t)n * esz, (size_t)pitch * esz, 0, (size_t)(pitch - n) * esz, (size_t)(nrow - 1), ctx().stream));
    return fir_filter_any(h, xp, (nrow - 1) * pitch + n, 0, yp);
}

int skdsp_fir_filter_rows(skdsp_handle hh, const void *x, int64_t n, int64_t nrow, void *y)
{
    API_BEGIN;
    FirHandle *h = as_handle<FirHandle>(hh, H_FIR);
    SK_CHECK(h, SKDSP_ERR_BADARG, "fir_filter_rows: not a FIR handle");
    SK_CHECK(n >= 0 && nrow >= 0 && nrow < ((int64_t)1 << 31), SKDSP_ERR_BADARG, "fir_filter_rows: bad arguments");
    if (n == 0 || nrow == 0) return SKDSP_OK;
    SK_CHECK(x && y, SKDSP_ERR_BADARG, "fir_filter_rows: null buffer");
    std::lock_guard<std::mutex> lk(h->mu);
    const size_t esz = dtype_size(h->dtype);
    const int64_t pitch = fir_rows_pitch(h, n);
    const size_t total = (size_t)nrow * (size_t)pitch * esz;
    // one block holds every row behind its zeros: refused beyond what a pitched copy takes / a sane staging budget (the caller then filters
    // row by row, each through the chunk pipeline)
    SK_CHECK((size_t)pitch * esz * 2 < ((size_t)1 << 31) && total <= kRowsBlockBudget, SKDSP_ERR_UNSUPPORTED,
             "fir_filter_rows: %lld rows of %lld samples do not fit one staged block (%zu bytes)", (long long)nrow, (long long)n, total);
    void *base = nullptr, *yp = nullptr;
    const bool wide = h->wide_out && !dtype_double(h->dtype);
    int rc = ws_reserve(0, kHeadroomBytes + (wide ? 2 : 1) * total + 256, &base);
    if (rc) return rc;
    void *xp = (char *)base + kHeadroomBytes;
    if ((rc = ws_reserve(1, total + 256, &yp))) return rc;
    SK_HIP(hipMemcpy2DAsync(xp, (size_t)pitch * esz, x, (size_t)n * esz, (size_t)n * esz, (size_t)nrow, hipMemcpyHostToDevice, ctx().stream));
    if ((rc = fir_rows_run(h, n, nrow, pitch, xp, yp))) return rc;
    size_t osz = esz;
    if (wide) {   // widen on the device (the staged input is done with in stream order)
        if ((rc = widen_launch(yp, (int64_t)(total / 4), xp, ctx().stream))) return rc;
        yp = xp;
        osz = 2 * esz;
    }
    SK_HIP(hipMemcpy2DAsync(y, (size_t)n * osz, yp, (size_t)pitch * osz, (size_t)n * osz, (size_t)nrow, hipMemcpyDeviceToHost, ctx().stream));
    return sync_checked();
}

int skdsp_fir_filter_rows_dev(skdsp_handle hh, const void *x_dev, int64_t n, int64_t nrow, int64_t x_stride, int64_t y_stride, void *y_dev)
{
    API_BEGIN;
    FirHandle *h = as_handle<FirHandle>(hh, H_FIR);
    SK_CHECK(h, SKDSP_ERR_BADARG, "fir_filter_rows: not a FIR handle");
    SK_CHECK(n >= 0 && nrow >= 0 && nrow < ((int64_t)1 << 31), SKDSP_ERR_BADARG, "fir_filter_rows: bad arguments");
    if (n == 0 || nrow == 0) return SKDSP_OK;
    SK_CHECK(x_stride >= n && y_stride >= n, SKDSP_ERR_BADARG, "fir_filter_rows: row stride below the row length");
    std::lock_guard<std::mutex> lk(h->mu);
    const size_t esz = dtype_size(h->dtype);
    const int64_t pitch = fir_rows_pitch(h, n);
    const size_t total = (size_t)nrow * (size_t)pitch * esz;
    SK_CHECK((size_t)pitch * esz < ((size_t)1 << 31) && (size_t)x_stride * esz < ((size_t)1 << 31) && (size_t)y_stride * esz < ((size_t)1 << 31) &&
                 total <= kRowsBlockBudget, SKDSP_ERR_UNSUPPORTED,
             "fir_filter_rows_dev: %lld rows of %lld samples do not fit one staged block (%zu bytes)", (long long)nrow, (long long)n, total);
    void *base = nullptr, *yp = nullptr;
    int rc = ws_reserve(0, kHeadroomBytes + total + 256, &base);
    if (rc) return rc;
    void *xp = (char *)base + kHeadroomBytes;
    if ((rc = ws_reserve(1, total + 256, &yp))) return rc;
    SK_HIP(hipMemcpy2DAsync(xp, (size_t)pitch * esz, x_dev, (size_t)x_stride * esz, (size_t)n * esz, (size_t)nrow, hipMemcpyDeviceToDevice, ctx().stream));
    if ((rc = fir_rows_run(h, n, nrow, pitch, xp, yp))) return rc;
    SK_HIP(hipMemcpy2DAsync(y_dev, (size_t)y_stride * esz, yp, (size_t)pitch * esz, (size_t)n * esz, (size_t)nrow, hipMemcpyDeviceToDevice, ctx().stream));
    return SKDSP_OK;
}

int skdsp_fir_filter(skdsp_handle h, const void *x, int64_t n, void *y) { return fir_host_call(h, x, n, 1, 1, 0, y); }

int skdsp_fir_filter_sharded(skdsp_handle h, const void *x, int64_t n, void *y, int ngpu)
{
    {
        API_BEGIN;
        SK_CHECK(ngpu >= 0 && ngpu <= slot_count(), SKDSP_ERR_BADARG, "fir_filter_sharded: ngpu = %d, %d slots bound (skdsp_init_devices)", ngpu,
                 slot_count());
    }
    return fir_host_call(h, x, n, 1, 1, 0, y, ngpu);   // (at most ngpu slots; 0: every bound one)
}
int skdsp_fir_up(skdsp_handle h, const void *x, int64_t n, int L, void *y) { return fir_host_call(h, x, n, L, 1, 1, y); }
int skdsp_fir_dn(skdsp_handle h, const void *x, int64_t n, int M, void *y) { return fir_host_call(h, x, n, 1, M, 1, y); }
int skdsp_fir_updn(skdsp_handle h, const void *x, int64_t n, int L, int M, void *y) { return fir_host_call(h, x, n, L, M, 1, y); }

}  // extern "C"
