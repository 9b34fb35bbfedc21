// iir_api.hip -- IIR dispatch and handle creation behind the extern "C" boundary (see include/skdsp.h).  The numerical
// host code of handle creation (factorisation, probes) is iir_design.hpp, which needs no device.
#include "api_internal.hpp"
#include "iir_design.hpp"
#include <cstring>

namespace skdsp {

// IIR on an interleaved-or-real device vector (handles the complex -> 2 planes detour).
// tmp slot 3 holds the planes.  y may alias x.
static int iir_any_dev(IirHandle *h, const void *x_dev, int64_t n, void *y_dev, const double *zi = nullptr, double *zf = nullptr)
{
    hipStream_t s = ctx().stream;
    if (n <= 0) {
        const size_t zb = (size_t)(dtype_complex(h->dtype) ? 2 : 1) * h->nsec * h->order * 8;
        if (zf && zi) memcpy(zf, zi, zb);
        else if (zf) memset(zf, 0, zb);
        return SKDSP_OK;
    }
    if (!dtype_complex(h->dtype)) return iir_launch_planar(h, x_dev, n, 1, 0, y_dev, s, zi, zf);
    const bool planar_only = opt().iir_planar != 0;  // developer A/B switch (and the tests)
    if (!planar_only && !h->groups.empty() && !h->twin64 && !zi && !zf && opt().iir_par > 0) {
        // more than 8 biquads on a complex signal: group after group in place behind the first, each through the parallel form on the
        // interleaved samples where it applies (else whatever that group's own dispatch takes) -- not the whole cascade through two planes
        for (size_t gi = 0; gi < h->groups.size(); ++gi) {
            IirHandle *g = h->groups[gi];
            const void *src = gi == 0 ? x_dev : y_dev;
            int rc = iir_par_launch(g, src, n, 1, 0, 0, y_dev, s, 1, 1, 1);
            if (rc == 1) rc = iir_any_dev(g, src, n, y_dev);
            if (rc) return rc;
        }
        return SKDSP_OK;
    }
    if (!planar_only) {
        // decaying filters: both components stay interleaved end to end (iir_k1c / iir_k3c kernels)
        const int r1 = iir_launch_planar(h, x_dev, n, 2, 0, y_dev, s, zi, zf, 1);
        if (r1 != 1) return r1;
    }
    const size_t rsz = dtype_double(h->dtype) ? 8 : 4;
    const int64_t stride = (int64_t)round_up((size_t)n, 64);
    void *planes = nullptr;
    int rc = ws_reserve(3, (size_t)2 * stride * rsz, &planes);
    if (rc) return rc;
    void *re = planes, *im = (char *)planes + (size_t)stride * rsz;
    if ((rc = deinterleave_launch(x_dev, n, h->dtype, re, im, s))) return rc;
    if ((rc = iir_launch_planar(h, planes, n, 2, stride, planes, s, zi, zf))) return rc;
    return interleave_launch(re, im, n, h->dtype, y_dev, s);
}

// y = filter(L * upsample(x, L)).  Real: zero-stuff straight into y, then filter in place.  Complex:
// zero-stuff straight into the two planes the scan works on (no stuffed interleaved copy, no
// deinterleave pass), filter, interleave into y.
static int iir_up_any(IirHandle *h, const void *x_dev, int64_t n, int L, void *y_dev)
{
    hipStream_t s = ctx().stream;
    const int64_t nl = n * L;
    if (nl <= 0) return SKDSP_OK;
    int rc;
    if (!dtype_complex(h->dtype)) {
        // the parallel-form kernel zero-stuffs while it stages a segment: the L-fold signal is never written (1 = not applicable)
        if (L > 1 && opt().iir_par && opt().iir_up_fused && h->order == 2) {
            rc = iir_par_launch(h, x_dev, nl, 1, 0, 0, y_dev, s, 1, 0, L);
            if (rc != 1) return rc;
        }
        if ((rc = upsample_launch(x_dev, n, L, h->dtype, (double)L, y_dev, s))) return rc;
        return iir_any_dev(h, y_dev, nl, y_dev);
    }
    if (L > 1 && opt().iir_par && opt().iir_up_fused && h->order == 2 && !opt().iir_planar) {   // (interleaved in, interleaved out)
        rc = iir_par_launch(h, x_dev, nl, 1, 0, 0, y_dev, s, 1, 1, L);
        if (rc != 1) return rc;
    }
    const size_t rsz = dtype_double(h->dtype) ? 8 : 4;
    const int64_t stride = (int64_t)round_up((size_t)nl, 64);
    void *planes = nullptr;
    if ((rc = ws_reserve(3, (size_t)2 * stride * rsz, &planes))) return rc;
    void *re = planes, *im = (char *)planes + (size_t)stride * rsz;
    if ((rc = upsample_planes_launch(x_dev, n, L, h->dtype, (double)L, re, im, s))) return rc;
    if ((rc = iir_launch_planar(h, planes, nl, 2, stride, planes, s))) return rc;
    return interleave_launch(re, im, nl, h->dtype, y_dev, s);
}

}  // namespace skdsp

using namespace skdsp;

extern "C" {

// ------------------------------------------------------------------------ IIR
// (b, a) -> sos rows through iir_design.hpp, its failure as this library reports errors
static int tf_factor(const double *b, int nb, const double *a, int na, std::vector<double> &sos, int *nsec)
{
    const char *msg = nullptr;
    SK_CHECK(tf_to_sos(b, nb, a, na, sos, nsec, &msg) == 0, SKDSP_ERR_UNSUPPORTED, msg, (int)std::max(nb, na) - 1);
    return SKDSP_OK;
}

// seq_limit > 0: the spread above which the handle runs the reference's recursion, given by the caller instead of derived from `dtype` -- the
// float64 twin of a float32 handle serves the float32 contract, so it is probed against the float32 limit its parent just passed (with the
// float64 limit a cheby1(26) cascade, spread 3.7e-11, would have run sample by sample although 1e-6 never needed it)
static int iir_create_common(int nsec, int order, const std::vector<double> &coef, int dtype, skdsp_handle *out, double seq_limit = 0.0)
{
    SK_CHECK(out, SKDSP_ERR_BADARG, "iir_create: null out");
    SK_CHECK(dtype_valid(dtype), SKDSP_ERR_BADARG, "iir_create: bad dtype %d", dtype);
    SK_CHECK(order == 2 && nsec >= 1 && nsec <= 4096, SKDSP_ERR_UNSUPPORTED,
             "iir_create: %d sections of order %d not supported (second-order sections, 1 .. 4096 of them)", nsec, order);
    std::unique_ptr<IirHandle> h(new IirHandle());
    h->kind = H_IIR;
    h->dtype = dtype;
    h->nsec = nsec;
    h->order = order;
    h->coef = coef;
    // 1. Sequential?  Cascades whose float64 result is itself uncertain beyond what the scans may add to it (cascade_spread) run the
    // recursion itself (iir_seq.hip): slow, and bit for bit the reference's result.  Cascades of up to 8 sections are not probed: the
    // parallel form's own acceptance test covers them.
    if (nsec > 8 && opt().iir_seq != 0) {
        h->seq_spread = cascade_spread(coef.data(), nsec);
        const double limit = seq_limit > 0.0 ? seq_limit : dtype_double(dtype) ? 2.5e-13 : 2.5e-9;   // (400 x spread stays inside the contract)
        if (opt().iir_seq == 2 || !(h->seq_spread <= limit)) {
            h->seq = true;
            h->seq_coef = coef;
            *out = h.release();
            return SKDSP_OK;
        }
    }
    // 2. More than 8 sections: groups of at most 8, each a handle of its own, made from the CALLER's factorisation -- unless the handle is
    // float32 and the rounding of the signal between the groups would break its contract (boundary_cost).  Such cascades keep the largest
    // groups the cascade kernels take (12: no boundary at all up to 12 sections)
    bool grouped = nsec > 8;
    if (grouped && !dtype_double(dtype) && !(boundary_cost(coef.data(), nsec) <= 16.0)) {
        if (nsec > 12) {
            // too many sections for one launch sequence, and no float32 boundary is safe: the same cascade in float64 (widen, filter, narrow)
            skdsp_handle th = nullptr;
            const int rc = iir_create_common(nsec, 2, coef, dtype == SKDSP_C64 ? SKDSP_C128 : SKDSP_F64, &th, 2.5e-9);
            if (rc) return rc;
            h->twin64 = static_cast<IirHandle *>(th);
            h->twin64->slot = ctx().slot;
            *out = h.release();
            return SKDSP_OK;
        }
        grouped = false;   // one launch sequence of the cascade kernels: float64 between ALL sections
    }
    if (grouped) {
        int s0 = 0;
        for (const int cnt : group_sizes(nsec, 8)) {
            std::vector<double> part(coef.begin() + (size_t)5 * s0, coef.begin() + (size_t)5 * (s0 + cnt));
            skdsp_handle gh = nullptr;
            const int rc = iir_create_common(cnt, 2, part, dtype, &gh);
            if (rc) return rc;
            IirHandle *gp = static_cast<IirHandle *>(gh);
            gp->group_first = s0;
            gp->slot = ctx().slot;
            h->groups.push_back(gp);
            s0 += cnt;
        }
        *out = h.release();
        return SKDSP_OK;
    }
    // 3. One launch sequence: the unit-tail re-factorisation where it applies
    h->unit_tail = unit_tail(h->coef.data(), nsec, h->state_scale);
    *out = h.release();
    return SKDSP_OK;
}

int skdsp_sos_create(const double *sos, int nsec, int dtype, skdsp_handle *out)
{
    API_BEGIN;
    SK_CHECK(sos && nsec >= 1, SKDSP_ERR_BADARG, "sos_create: sos array must be shape (n_sections, 6)");
    std::vector<double> coef;
    SK_CHECK(sos_rows_to_coef(sos, nsec, coef), SKDSP_ERR_BADARG, "sos[:, 3] should be all ones");
    return iir_create_common(nsec, 2, coef, dtype, out);
}

int skdsp_iir_sequential(skdsp_handle hh, int *is_sequential, double *spread)
{
    HandleBase *hb = static_cast<HandleBase *>(hh);
    SK_CHECK(hb && hb->kind == H_IIR, SKDSP_ERR_BADARG, "iir_sequential: not an IIR handle");
    IirHandle *h = static_cast<IirHandle *>(hb);
    if (is_sequential) *is_sequential = (h->seq || (h->twin64 && h->twin64->seq)) ? 1 : 0;   // (what actually runs: a float32 handle may filter through its float64 twin)
    if (spread) *spread = h->seq_spread;
    return SKDSP_OK;
}

int skdsp_tf2sos(const double *b, int nb, const double *a, int na, double *sos_out, int *nsec_out)
{
    // host-only helper (no GPU needed): the factorisation skdsp_tf_create applies
    SK_CHECK(b && a && nb >= 1 && na >= 1 && sos_out && nsec_out, SKDSP_ERR_BADARG, "tf2sos: bad arguments");
    SK_CHECK(a[0] != 0.0, SKDSP_ERR_BADARG, "tf2sos: a[0] must be nonzero");
    std::vector<double> sos;
    int nsec = 0;
    int rc = tf_factor(b, nb, a, na, sos, &nsec);
    if (rc) return rc;
    memcpy(sos_out, sos.data(), sos.size() * sizeof(double));
    *nsec_out = nsec;
    return SKDSP_OK;
}

int skdsp_tf_create(const double *b, int nb, const double *a, int na, int dtype, skdsp_handle *out)
{
    API_BEGIN;
    SK_CHECK(b && a && nb >= 1 && na >= 1, SKDSP_ERR_BADARG, "tf_create: need b and a");
    SK_CHECK(a[0] != 0.0, SKDSP_ERR_BADARG, "tf_create: a[0] must be nonzero");
    std::vector<double> sos;
    int nsec = 0;
    int rc = tf_factor(b, nb, a, na, sos, &nsec);
    if (rc) return rc;
    std::vector<double> coef;
    sos_rows_to_coef(sos.data(), nsec, coef);   // (tf_to_sos writes sos[:, 3] = 1)
    return iir_create_common(nsec, 2, coef, dtype, out);
}

int skdsp_iir_filter_dev(skdsp_handle hh, const void *x_dev, int64_t n, void *y_dev)
{
    API_BEGIN;
    IirHandle *h = as_handle<IirHandle>(hh, H_IIR);
    SK_CHECK(h, SKDSP_ERR_BADARG, "iir_filter: not an IIR handle");
    std::lock_guard<std::mutex> lk(h->mu);
    return iir_any_dev(h, x_dev, n, y_dev);
}

int skdsp_sos_par_info(const double *sos, int nsec, double *out, int *accepted)
{
    SK_CHECK(sos && out && accepted, SKDSP_ERR_BADARG, "sos_par_info: null argument");
    SK_CHECK(nsec >= 1 && nsec <= 8, SKDSP_ERR_UNSUPPORTED, "sos_par_info: 1..8 biquads");
    std::vector<double> coef;
    SK_CHECK(sos_rows_to_coef(sos, nsec, coef), SKDSP_ERR_BADARG, "sos[:, 3] should be all ones");
    return iir_par_expand_host(coef.data(), nsec, out, accepted);
}

// rows of one launch (parallel form) or, where that does not apply, row by row through the cascade kernels
static int iir_rows_dev(IirHandle *h, const void *x_dev, int64_t n, int64_t nrow, int64_t x_stride, int64_t y_stride, void *y_dev)
{
    if (n <= 0 || nrow <= 0) return SKDSP_OK;
    SK_CHECK(x_stride >= n && y_stride >= n, SKDSP_ERR_BADARG, "iir_filter_rows: row stride below the row length");
    SK_CHECK(nrow < (1 << 24), SKDSP_ERR_BADARG, "iir_filter_rows: too many rows");
    const size_t esz = dtype_size(h->dtype);
    // the reference's recursion takes all rows in ONE launch (one wave per row), not one single-wave kernel per row in stream order
    if (h->seq && !dtype_complex(h->dtype)) return iir_seq_launch(h, x_dev, n, (int)nrow, x_stride, y_stride, y_dev, ctx().stream);
    if (!h->groups.empty() && !dtype_complex(h->dtype) && opt().iir_par > 0) {
        // groups of sections (more than 8 biquads): every group over all rows in one launch where its parallel form applies, in place behind the first
        for (size_t gi = 0; gi < h->groups.size(); ++gi) {
            IirHandle *g = h->groups[gi];
            const void *src = gi == 0 ? x_dev : y_dev;
            const int64_t ss = gi == 0 ? x_stride : y_stride;
            int rc = iir_par_launch(g, src, n, (int)nrow, ss, y_stride, y_dev, ctx().stream);
            if (rc == 1) {
                for (int64_t r = 0; r < nrow; ++r)
                    if ((rc = iir_any_dev(g, (const char *)src + (size_t)r * ss * esz, n, (char *)y_dev + (size_t)r * y_stride * esz))) return rc;
            } else if (rc) {
                return rc;
            }
        }
        return SKDSP_OK;
    }
    if (!dtype_complex(h->dtype) && opt().iir_par > 0) {
        const int r = iir_par_launch(h, x_dev, n, (int)nrow, x_stride, y_stride, y_dev, ctx().stream);
        if (r != 1) return r;
    }
    for (int64_t r = 0; r < nrow; ++r) {
        const int rc = iir_any_dev(h, (const char *)x_dev + (size_t)r * x_stride * esz, n, (char *)y_dev + (size_t)r * y_stride * esz);
        if (rc) return rc;
    }
    return SKDSP_OK;
}

int skdsp_iir_filter_rows_dev(skdsp_handle hh, const void *x_dev, int64_t n, int64_t nrow, int64_t x_stride, int64_t y_stride, void *y_dev)
{
    API_BEGIN;
    IirHandle *h = as_handle<IirHandle>(hh, H_IIR);
    SK_CHECK(h, SKDSP_ERR_BADARG, "iir_filter_rows: not an IIR handle");
    std::lock_guard<std::mutex> lk(h->mu);
    return iir_rows_dev(h, x_dev, n, nrow, x_stride, y_stride, y_dev);
}

int skdsp_iir_filter_rows(skdsp_handle hh, const void *x, int64_t n, int64_t nrow, void *y)
{
    API_BEGIN;
    IirHandle *h = as_handle<IirHandle>(hh, H_IIR);
    SK_CHECK(h, SKDSP_ERR_BADARG, "iir_filter_rows: not an IIR handle");
    SK_CHECK(n >= 0 && nrow >= 0, SKDSP_ERR_BADARG, "iir_filter_rows: bad arguments");
    if (n == 0 || nrow == 0) return SKDSP_OK;
    SK_CHECK(x && y, SKDSP_ERR_BADARG, "iir_filter_rows: null buffer");
    std::lock_guard<std::mutex> lk(h->mu);
    const size_t esz = dtype_size(h->dtype), bytes = (size_t)n * (size_t)nrow * esz;
    void *x_dev = nullptr, *y_dev = nullptr;
    int rc = stage_in(x, bytes, &x_dev);
    if (rc) return rc;
    if ((rc = ws_reserve(1, bytes + 256, &y_dev))) return rc;
    if ((rc = iir_rows_dev(h, x_dev, n, nrow, n, n, y_dev))) return rc;
    return stage_out(y, y_dev, bytes, h);
}

int skdsp_iir_state_len(skdsp_handle hh, int *len)
{
    IirHandle *h = as_handle<IirHandle>(hh, H_IIR);
    SK_CHECK(h && len, SKDSP_ERR_BADARG, "iir_state_len: not an IIR handle");
    *len = (dtype_complex(h->dtype) ? 2 : 1) * h->nsec * h->order;
    return SKDSP_OK;
}

int skdsp_iir_filter_state_dev(skdsp_handle hh, const void *x_dev, int64_t n, const double *zi, double *zf, void *y_dev)
{
    API_BEGIN;
    IirHandle *h = as_handle<IirHandle>(hh, H_IIR);
    SK_CHECK(h, SKDSP_ERR_BADARG, "iir_filter_state: not an IIR handle");
    std::lock_guard<std::mutex> lk(h->mu);
    return iir_any_dev(h, x_dev, n, y_dev, zi, zf);
}

int skdsp_iir_up_dev(skdsp_handle hh, const void *x_dev, int64_t n, int L, void *y_dev)
{
    API_BEGIN;
    IirHandle *h = as_handle<IirHandle>(hh, H_IIR);
    SK_CHECK(h, SKDSP_ERR_BADARG, "iir_up: not an IIR handle");
    SK_CHECK(L >= 1, SKDSP_ERR_BADARG, "iir_up: L must be >= 1");
    std::lock_guard<std::mutex> lk(h->mu);
    return iir_up_any(h, x_dev, n, L, y_dev);
}

// y = downsample(filter(x), M) on device vectors (both the _dev and the host-pointer entry use it)
static int iir_dn_any(IirHandle *h, const void *x_dev, int64_t n, int M, void *y_dev)
{
    if (n <= 0) return SKDSP_OK;
    // K3 stores every M-th output itself -- the full-rate result never reaches HBM
    if (M > 1 && M <= 4096 && !opt().iir_dn_full) {
        if (!dtype_complex(h->dtype)) return iir_launch_planar(h, x_dev, n, 1, 0, y_dev, ctx().stream, nullptr, nullptr, 0, M);
        if (!opt().iir_planar) {  // interleaved complex kernels (decaying filters); 1 = not applicable
            const int r1 = iir_launch_planar(h, x_dev, n, 2, 0, y_dev, ctx().stream, nullptr, nullptr, 1, M);
            if (r1 != 1) return r1;
        }
    }
    void *full = nullptr;
    int rc = ws_reserve(2, (size_t)n * dtype_size(h->dtype) + 256, &full);
    if (rc) return rc;
    if ((rc = iir_any_dev(h, x_dev, n, full))) return rc;
    return downsample_launch(full, n, M, 0, h->dtype, y_dev, ctx().stream);
}

int skdsp_iir_dn_dev(skdsp_handle hh, const void *x_dev, int64_t n, int M, void *y_dev)
{
    API_BEGIN;
    IirHandle *h = as_handle<IirHandle>(hh, H_IIR);
    SK_CHECK(h, SKDSP_ERR_BADARG, "iir_dn: not an IIR handle");
    SK_CHECK(M >= 1, SKDSP_ERR_BADARG, "iir_dn: M must be >= 1");
    std::lock_guard<std::mutex> lk(h->mu);
    return iir_dn_any(h, x_dev, n, M, y_dev);
}

struct IirChunkJob {
    IirHandle *h;
    std::vector<double> state;  // state after the previous chunk, in the caller-visible (scipy zi) convention
};
static int iir_chunk_kernel(void *self, const void *x_dev, int64_t n_k, int64_t, void *y_dev, int64_t k)
{
    IirChunkJob *j = static_cast<IirChunkJob *>(self);
    std::vector<double> zf(j->state.size());
    int rc = iir_any_dev(j->h, x_dev, n_k, y_dev, k == 0 ? nullptr : j->state.data(), zf.data());
    j->state.swap(zf);
    return rc;
}
static void *iir_job_on_slot(void *base, int) { return base; }

static int iir_host_call(skdsp_handle hh, const void *x, int64_t n, int L, int M, void *y)
{
    API_BEGIN;
    IirHandle *h = as_handle<IirHandle>(hh, H_IIR);
    SK_CHECK(h, SKDSP_ERR_BADARG, "iir: not an IIR handle");
    SK_CHECK(n >= 0 && L >= 1 && M >= 1, SKDSP_ERR_BADARG, "iir: bad arguments");
    const size_t esz = dtype_size(h->dtype);
    const int64_t n_out = (n * L) / M;
    if (n_out == 0) return SKDSP_OK;  // fewer than M samples: nothing to deliver (y may be NULL)
    SK_CHECK(x && y, SKDSP_ERR_BADARG, "iir: null buffer");
    std::lock_guard<std::mutex> lk(h->mu);
    if (L == 1 && M == 1 && opt().host_pipeline && n > (((int64_t)3 << opt().host_chunk_log2) >> 1)) {
        // long vector: chunk pipeline on the caller's slot, the recursion carried from chunk to chunk as zi / zf
        const ChunkPlan p = plan_chunks(n, 1, 1, 0, esz, h->wide_out && !dtype_double(h->dtype), opt().host_chunk_log2);
        IirChunkJob job;
        job.h = h;
        job.state.assign((size_t)(dtype_complex(h->dtype) ? 2 : 1) * h->nsec * h->order, 0.0);
        return run_on_slots(p, (const char *)x, (char *)y, iir_chunk_kernel, iir_job_on_slot, &job, false);
    }
    void *x_dev = nullptr, *y_dev = nullptr;
    int rc = stage_in(x, (size_t)n * esz, &x_dev);
    if (rc) return rc;
    if (L > 1) {
        if ((rc = ws_reserve(1, (size_t)n * L * esz + 256, &y_dev))) return rc;
        if ((rc = iir_up_any(h, x_dev, n, L, y_dev))) return rc;
    } else if (M > 1) {
        if ((rc = ws_reserve(1, (size_t)n_out * esz + 256, &y_dev))) return rc;
        if ((rc = iir_dn_any(h, x_dev, n, M, y_dev))) return rc;  // K3 stores every M-th output itself
    } else {
        if ((rc = ws_reserve(1, (size_t)n * esz + 256, &y_dev))) return rc;
        if ((rc = iir_any_dev(h, x_dev, n, y_dev))) return rc;
    }
    return stage_out(y, y_dev, (size_t)n_out * esz, h);
}

int skdsp_iir_filter(skdsp_handle h, const void *x, int64_t n, void *y) { return iir_host_call(h, x, n, 1, 1, y); }
int skdsp_iir_up(skdsp_handle h, const void *x, int64_t n, int L, void *y) { return iir_host_call(h, x, n, L, 1, y); }
int skdsp_iir_dn(skdsp_handle h, const void *x, int64_t n, int M, void *y) { return iir_host_call(h, x, n, 1, M, y); }
// (SURVEY.md 8(b)'s names for the same three calls)
int skdsp_sos_filter(skdsp_handle h, const void *x, int64_t n, void *y) { return skdsp_iir_filter(h, x, n, y); }
int skdsp_sos_up(skdsp_handle h, const void *x, int64_t n, int L, void *y) { return skdsp_iir_up(h, x, n, L, y); }
int skdsp_sos_dn(skdsp_handle h, const void *x, int64_t n, int M, void *y) { return skdsp_iir_dn(h, x, n, M, y); }

}  // extern "C"
