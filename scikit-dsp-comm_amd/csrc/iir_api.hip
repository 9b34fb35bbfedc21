// iir_api.hip -- IIR handle creation and dispatch behind the extern "C" boundary (see include/skdsp.h), and all of the IIR host side that is
// not a launch: the plan of the cascade scans on the device, the workspaces, the state transfer, and iir_run, which executes the ONE routing
// decision of a call (iir_route.hpp).  The numerical host code needs no device: iir_design.hpp (factorisation, probes), iir_scan_plan.hpp.
#include "api_internal.hpp"
#include "iir_common.hpp"
#include "iir_design.hpp"
#include "iir_route.hpp"
#include <cstring>

namespace skdsp {

static_assert(SKDSP_F32 == kIirF32 && SKDSP_C64 == kIirC64 && SKDSP_F64 == kIirF64 && SKDSP_C128 == kIirC128, "iir_route.hpp mirrors the dtype codes");

IirHandle::~IirHandle()
{
    for (IirHandle *g : groups) delete g;
    delete twin64;
}

// ---- the plan of the cascade scans: the numbers are iir_scan_plan.hpp, here their device copies ---------------------------------
static int ensure_plan(IirHandle *h)
{
    if (h->plan) return SKDSP_OK;
    std::unique_ptr<IirPlan> p(new IirPlan());
    p->nsec = h->nsec; p->order = h->order; p->D = h->nsec * h->order;
    const size_t D = p->D;
    p->A_host = scan_A_host(h->coef.data(), h->nsec, h->order);
    int rc;
    if ((rc = p->pw_dev.alloc(kPowers * D * D)) || (rc = p->pwa_dev.alloc(8 * 4 * 64)) || (rc = p->lb_dev.alloc(8 * D * D)) ||
        (rc = p->lbk_dev.alloc(32 * D * D)) || (rc = p->state_dev.alloc(4 * D)) || (rc = p->agg_dev.alloc(2 * 2 * kMaxW * D)))
        return rc;
    h->plan = std::move(p);
    return SKDSP_OK;
}

// the tables of chunk length T on the device (cached: one chunk length at a time)
static int ensure_powers(IirHandle *h, int64_t T, hipStream_t s)
{
    IirPlan *p = iir_plan_of(h);
    if (p->cached_T == T) return SKDSP_OK;
    const ScanTables t = scan_tables(h->coef.data(), h->nsec, h->order, p->A_host, T, dtype_double(h->dtype));
    p->cached_T = -1;   // from the first overwrite until all tables are those of T, the plan holds the tables of no chunk length
    p->gt_T = -1;
    SK_HIP(hipMemcpyAsync(p->lbk_dev.dev, t.lbk.data(), t.lbk.size() * 8, hipMemcpyHostToDevice, s));
    if (t.gt_T == T) {
        const int rc = p->gt_dev.reserve(t.gt.size() * 8, s);
        if (rc) return rc;
        SK_HIP(hipMemcpyAsync(p->gt_dev.dev, t.gt.data(), t.gt.size() * 8, hipMemcpyHostToDevice, s));
    }
    p->n_lv = t.n_lv;
    p->n_lb = t.n_lb;
    SK_HIP(hipMemcpyAsync(p->lb_dev.dev, t.lb.data(), t.lb.size() * 8, hipMemcpyHostToDevice, s));
    SK_HIP(hipMemcpyAsync(p->pw_dev.dev, t.pw.data(), t.pw.size() * 8, hipMemcpyHostToDevice, s));
    SK_HIP(hipMemcpyAsync(p->pwa_dev.dev, t.pwa.data(), t.pwa.size() * 8, hipMemcpyHostToDevice, s));
    SK_HIP(hipStreamSynchronize(s));  // t is a local
    if (t.gt_T == T) p->gt_T = T;
    p->cached_T = T;
    return SKDSP_OK;
}

// ---- one decision per call (iir_route.hpp), and what it asks ----------------------------------------------------------------------
struct IirQueries {
    hipStream_t s;
    ParChoice par(IirHandle *h, bool interleaved, int nrow, int dec, int up, int64_t n) { return iir_par_takes(h, n, nrow, dec, interleaved, up, s); }
    int fused_cached(IirHandle *h, bool interleaved, int &fstate, int &fnlv)
    {
        const int rc = ensure_plan(h);
        if (rc) return rc;
        fstate = interleaved ? iir_plan_of(h)->fused_state_c : iir_plan_of(h)->fused_state;   // applicability only (cached); the policy is per call
        fnlv = interleaved ? iir_plan_of(h)->fused_nlv_c : iir_plan_of(h)->fused_nlv;
        return SKDSP_OK;
    }
    void fused_remember(IirHandle *h, bool interleaved, int fstate, int fnlv)
    {
        (interleaved ? iir_plan_of(h)->fused_state_c : iir_plan_of(h)->fused_state) = fstate;
        (interleaved ? iir_plan_of(h)->fused_nlv_c : iir_plan_of(h)->fused_nlv) = fnlv;
    }
    int scan_facts(IirHandle *h, int64_t T, ScanFacts &f)
    {
        const int rc = ensure_powers(h, T, s);
        f = ScanFacts{iir_plan_of(h)->n_lv, iir_plan_of(h)->n_lb, iir_plan_of(h)->gt_T};
        return rc;
    }
};
typedef IirStep<IirHandle> Step;

// the single pass or the two-pass scan of one handle: tables, chunk states, the state transfer, the launch.
// zi / zf: [nbatch][D] host states in the caller's factorisation
static int scan_step(const Step &st, const void *x, void *y, const double *zi_host, double *zf_host, hipStream_t s)
{
    IirHandle *h = st.h;
    const bool fused = st.engine == kEngFused, dbl = dtype_double(h->dtype);
    const int nbatch = st.nrow, dec = st.dec;
    const int64_t n = st.n;
    int rc = ensure_plan(h);
    if (rc) return rc;
    IirPlan *p = iir_plan_of(h);
    const int D = p->D;
    const int64_t T = fused ? fused_chunk(dbl, st.interleaved) : st.geom.T;
    if ((rc = ensure_powers(h, T, s))) return rc;   // (a no-op where the route asked for these tables last)
    if ((rc = p->v_dev.reserve(fused ? 0 : (size_t)nbatch * D * st.geom.J * 8, s))) return rc;
    SK_CHECK(dec <= 1 || (zf_host == nullptr && (st.interleaved || nbatch == 1)), SKDSP_ERR_UNSUPPORTED,
             "iir: decimating store needs a real or interleaved complex signal and no state output");
    SK_CHECK(nbatch >= 1 && nbatch <= 2, SKDSP_ERR_BADARG, "iir: batch must be 1 or 2");
    const double *zi_dev = nullptr;
    double *zf_dev = zf_host ? p->state_dev.dev + 2 * D : nullptr;
    if (zi_host) {
        std::vector<double> zi_int;  // the caller's DF2T states in the internal factorisation (IirHandle::state_scale)
        if (!h->state_scale.empty()) {
            zi_int.resize((size_t)nbatch * D);
            for (int b = 0; b < nbatch; ++b)
                for (int d = 0; d < D; ++d) zi_int[(size_t)b * D + d] = zi_host[(size_t)b * D + d] * h->state_scale[d];
            zi_host = zi_int.data();
        }
        SK_HIP(hipMemcpyAsync(p->state_dev.dev, zi_host, (size_t)nbatch * D * 8, hipMemcpyHostToDevice, s));
        if (!zi_int.empty()) SK_HIP(hipStreamSynchronize(s));  // zi_int is a local
        zi_dev = p->state_dev.dev;
    }
    if (fused) {
        rc = iir_fused_launch(h, x, n, nbatch, st.x_stride, y, zi_dev, zf_dev, s, dec, st.interleaved);
    } else {
        IirArgs a;
        a.x = x; a.y = y; a.n = n; a.T = T; a.J = st.geom.J; a.batch_stride = st.x_stride;
        a.il = st.interleaved ? 1 : 0;
        a.pw = p->pw_dev.dev; a.v = p->v_dev.as<double>();
        a.agg = p->agg_dev.dev;
        a.carry = p->agg_dev.dev + (size_t)2 * kMaxW * D;
        a.lbmat = p->lb_dev.dev;
        a.n_lb = st.fast ? 0 : p->n_lb;   // (aggregate-free mode: K3 reads the carries)
        a.n_lv = p->n_lv < 8 ? p->n_lv : 8;
        a.zi = zi_dev; a.zf = zf_dev;
        a.dec = dec > 1 ? dec : 1;
        a.n_keep = (n / a.dec) * a.dec;
        a.dec_dq = scan_dec_dq(st.interleaved, dbl, T, a.dec);
        a.dec_dr = scan_dec_dr(st.interleaved, dbl, T, a.dec);
        const ScanLaunch L{h->coef.data(), h->nsec, h->order, p->gt_dev.as<double>(), p->lbk_dev.dev, p->n_lv, p->gt_T, nbatch, st.geom.W, ctx().num_cus,
                           ScanForm{st.fast, h->unit_tail, scan_k1(st.fast, st.interleaved, D, T)}};
        rc = dbl ? iir_scan_launch_f64(L, a, s) : iir_scan_launch_f32(L, a, s);
        if (!rc) note_path("iir_scan");   // (recorded once the two-pass kernels WERE launched: the other engines note themselves)
    }
    if (rc) return rc;
    if (zf_host) {
        SK_HIP(hipMemcpyAsync(zf_host, zf_dev, (size_t)nbatch * D * 8, hipMemcpyDeviceToHost, s));
        SK_HIP(hipStreamSynchronize(s));
        if (!h->state_scale.empty())
            for (int b = 0; b < nbatch; ++b)
                for (int d = 0; d < D; ++d) zf_host[(size_t)b * D + d] /= h->state_scale[d];
    }
    return SKDSP_OK;
}

// one step of a route on row `row` of the call
static int run_step(const Step &st, const IirCall &c, size_t esz, const void *x_dev, void *y_dev, int64_t row, const double *zi, double *zf)
{
    hipStream_t s = ctx().stream;
    IirHandle *h = st.h;
    auto at = [&](const IirBuf<IirHandle> &b, void **out) -> int {
        auto owned = [&](DevBuffer &buf) {   // a buffer of the handle b.owner
            const int rc = buf.reserve((size_t)b.bytes, s);
            *out = buf.dev;
            return rc;
        };
        switch (b.kind) {
        case kBufX: *out = (char *)const_cast<void *>(x_dev) + (size_t)row * c.x_stride * esz; return SKDSP_OK;
        case kBufY: *out = (char *)y_dev + (size_t)row * c.y_stride * esz; return SKDSP_OK;
        case kBufPlanes: return ws_reserve(3, (size_t)b.bytes, out);
        case kBufFull: return ws_reserve(2, (size_t)b.bytes, out);
        case kBufGroupTmp: return owned(b.owner->group_tmp);
        case kBufTwinIn: return owned(b.owner->twin_in);
        default: return owned(b.owner->twin_out);
        }
    };
    void *src = nullptr, *dst = nullptr;
    int rc;
    if ((rc = at(st.src, &src)) || (rc = at(st.dst, &dst))) return rc;
    const size_t rsz = dtype_double(h->dtype) ? 8 : 4;
    auto im_of = [&](void *re, int64_t n) { return (void *)((char *)re + (size_t)(n + 63) / 64 * 64 * rsz); };
    switch (st.engine) {
    case kEngPar: return iir_par_launch(h, st.par, src, st.n, st.nrow, st.x_stride, st.y_stride, dst, s, st.dec, st.interleaved, st.up);
    case kEngWiden: return convert_launch(src, dst, st.n, true, s);
    case kEngNarrow: return convert_launch(src, dst, st.n, false, s);
    case kEngZeroStuff: return upsample_launch(src, st.n, st.up, h->dtype, (double)st.up, dst, s);
    case kEngZeroStuffPlanes: return upsample_planes_launch(src, st.n, st.up, h->dtype, (double)st.up, dst, im_of(dst, st.n * st.up), s);
    case kEngDeinterleave: return deinterleave_launch(src, st.n, h->dtype, dst, im_of(dst, st.n), s);
    case kEngInterleave: return interleave_launch(src, im_of(src, st.n), st.n, h->dtype, dst, s);
    case kEngDownsample: return downsample_launch(src, st.n, st.dec, 0, h->dtype, dst, s);
    default: break;
    }
    // iir_seq, iir_fused, the two-pass scan: they take and leave states -- of a group, its sections' slice of the caller's vectors
    const int Dg = h->nsec * h->order;
    const bool whole = Dg == st.state_D;
    std::vector<double> zi_g, zf_g;
    const double *zi_p = st.zi ? zi : nullptr;
    double *zf_p = st.zf ? zf : nullptr;
    if (zi_p && !whole) {
        zi_g.resize((size_t)st.nrow * Dg);
        for (int b = 0; b < st.nrow; ++b) memcpy(zi_g.data() + (size_t)b * Dg, zi + (size_t)b * st.state_D + h->order * st.state_first, (size_t)Dg * 8);
        zi_p = zi_g.data();
    }
    if (zf_p && !whole) {
        zf_g.assign((size_t)st.nrow * Dg, 0.0);
        zf_p = zf_g.data();
    }
    if (st.engine == kEngSeq) rc = iir_seq_launch(h, src, st.n, st.nrow, st.x_stride, st.y_stride, dst, s, zi_p, zf_p, st.dec);
    else rc = scan_step(st, src, dst, zi_p, zf_p, s);
    if (rc) return rc;
    if (zf_p && !whole)
        for (int b = 0; b < st.nrow; ++b) memcpy(zf + (size_t)b * st.state_D + h->order * st.state_first, zf_g.data() + (size_t)b * Dg, (size_t)Dg * 8);
    return SKDSP_OK;
}

// decide, then execute.  x / y: device vectors (y may alias x for .filter); zi / zf: the caller's host states
static int iir_run(IirHandle *h, IirCall c, const void *x_dev, void *y_dev, const double *zi = nullptr, double *zf = nullptr)
{
    c.zi = zi != nullptr; c.zf = zf != nullptr;
    c.num_cus = ctx().num_cus;
    const IirRouteOptions o{opt().iir_par, opt().iir_planar, opt().iir_up_fused, opt().iir_dn_full, opt().iir_two_pass, opt().iir_no_mfma};
    IirQueries q{ctx().stream};
    const IirRoute<IirHandle> r = iir_route(h, c, o, q);
    SK_CHECK(r.status != kIirNoRoute, SKDSP_ERR_UNSUPPORTED, "iir: no engine takes this call");
    if (r.status) return r.status;   // (a query failed and said why)
    const size_t esz = dtype_size(h->dtype);
    for (size_t i = 0; i < r.steps.size();) {
        const size_t block = r.steps[i].block > 0 ? (size_t)r.steps[i].block : 1;
        const int64_t rows = r.steps[i].block > 0 ? c.nrow : 1;
        for (int64_t row = 0; row < rows; ++row)
            for (size_t j = i; j < i + block; ++j)
                if (int rc = run_step(r.steps[j], c, esz, x_dev, y_dev, row, zi, zf)) return rc;
        i += block;
    }
    return SKDSP_OK;
}

// IIR on an interleaved-or-real device vector.  y may alias x.
static int iir_any_dev(IirHandle *h, const void *x_dev, int64_t n, void *y_dev, const double *zi = nullptr, double *zf = nullptr)
{
    if (n <= 0) {
        const size_t zb = (size_t)(dtype_complex(h->dtype) ? 2 : 1) * h->nsec * h->order * 8;
        if (zf && zi) memcpy(zf, zi, zb);
        else if (zf) memset(zf, 0, zb);
        return SKDSP_OK;
    }
    IirCall c;
    c.kind = kIirFilter; c.n = n;
    return iir_run(h, c, x_dev, y_dev, zi, zf);
}

// y = filter(L * upsample(x, L))
static int iir_up_any(IirHandle *h, const void *x_dev, int64_t n, int L, void *y_dev)
{
    if (n * L <= 0) return SKDSP_OK;
    IirCall c;
    c.kind = kIirUp; c.n = n; c.rate = L;
    return iir_run(h, c, x_dev, y_dev);
}

// y = downsample(filter(x), M) on device vectors (both the _dev and the host-pointer entry use it)
static int iir_dn_any(IirHandle *h, const void *x_dev, int64_t n, int M, void *y_dev)
{
    if (n <= 0) return SKDSP_OK;
    IirCall c;
    c.kind = kIirDn; c.n = n; c.rate = M;
    return iir_run(h, c, x_dev, y_dev);
}

static int iir_rows_dev(IirHandle *h, const void *x_dev, int64_t n, int64_t nrow, int64_t x_stride, int64_t y_stride, void *y_dev)
{
    if (n <= 0 || nrow <= 0) return SKDSP_OK;
    SK_CHECK(x_stride >= n && y_stride >= n, SKDSP_ERR_BADARG, "iir_filter_rows: row stride below the row length");
    SK_CHECK(nrow < (1 << 24), SKDSP_ERR_BADARG, "iir_filter_rows: too many rows");
    IirCall c;
    c.kind = kIirRows; c.n = n; c.nrow = nrow; c.x_stride = x_stride; c.y_stride = y_stride;
    return iir_run(h, c, x_dev, y_dev);
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
    StagePlan p;
    p.input(x, bytes);
    const int iy = p.add_out(y, bytes);
    int rc = stage_begin(p);
    if (rc) return rc;
    return stage_finish(p, iir_rows_dev(h, p.in_dev(), n, nrow, n, n, p.dev(iy)), h);
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
    StagePlan p;
    p.input(x, (size_t)n * esz);
    const int iy = p.add_out(y, (size_t)n_out * esz);   // (the callers pass L = 1 or M = 1: n L, n / M or n samples)
    int rc = stage_begin(p);
    if (rc) return rc;
    if (L > 1) rc = iir_up_any(h, p.in_dev(), n, L, p.dev(iy));
    else if (M > 1) rc = iir_dn_any(h, p.in_dev(), n, M, p.dev(iy));  // K3 stores every M-th output itself
    else rc = iir_any_dev(h, p.in_dev(), n, p.dev(iy));
    return stage_finish(p, rc, h);
}

int skdsp_iir_filter(skdsp_handle h, const void *x, int64_t n, void *y) { return iir_host_call(h, x, n, 1, 1, y); }
int skdsp_iir_up(skdsp_handle h, const void *x, int64_t n, int L, void *y) { return iir_host_call(h, x, n, L, 1, y); }
int skdsp_iir_dn(skdsp_handle h, const void *x, int64_t n, int M, void *y) { return iir_host_call(h, x, n, 1, M, y); }
// (SURVEY.md 8(b)'s names for the same three calls)
int skdsp_sos_filter(skdsp_handle h, const void *x, int64_t n, void *y) { return skdsp_iir_filter(h, x, n, y); }
int skdsp_sos_up(skdsp_handle h, const void *x, int64_t n, int L, void *y) { return skdsp_iir_up(h, x, n, L, y); }
int skdsp_sos_dn(skdsp_handle h, const void *x, int64_t n, int M, void *y) { return skdsp_iir_dn(h, x, n, M, y); }

}  // extern "C"
