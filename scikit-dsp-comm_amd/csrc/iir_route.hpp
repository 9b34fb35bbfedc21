// iir_route.hpp -- which engines an IIR call runs, in which order, on which buffers: ONE decision per call, complete before the call's first
// kernel is launched, which iir_api.hip (iir_run) executes.  Standard headers only: tests/host/iir_route_emul.cpp walks it on the host over
// the recorded table tests/iir_routes/mi355x.txt.  An engine that appears in a route applies; every *_launch checks its own rule again.
//
// The order of the attempts is the dispatch's history and is kept as it was:
//   a handle is sequential (iir_seq), a float64 twin (widen / the twin's route / narrow), a chain of groups, or one launch sequence;
//   one launch sequence: the parallel form (no state in or out), else the single pass (iir_fused), else the two-pass scan;
//   complex signals: interleaved where the engines take them (the parallel form, the single pass, the aggregate-free two-pass kernels),
//   else through two planes; grouped complex handles with no state and no twin take the parallel form group by group on the interleaved signal;
//   .up: the parallel form zero-stuffs while it stages, else zero-stuff then filter; .dn: the decimating store of the engines for M <= 4096,
//   else filter at full rate then downsample; rows: one launch of the parallel form (per group), else row by row.
// Facts that cost something are asked through the query object Q, each at most once per call:
//   ParChoice par(h, interleaved, nrow, dec, up, n)            does the parallel form take this call (plan on first use + par_choose)
//   int fused_cached(h, interleaved, &fstate, &fnlv)          the cached single-pass applicability of the handle (0 untested, 1, -1)
//   void fused_remember(h, interleaved, fstate, fnlv)
//   int scan_facts(h, T, &facts)                              n_lv / n_lb / gt_T of the tables at chunk length T (makes them)
// (the int answers are 0 or a negative error code, which ends the route).
#pragma once
#include <cstdint>
#include <vector>
#include "iir_par_plan.hpp"
#include "iir_scan_plan.hpp"

namespace skdsp {

enum { kIirF32 = 0, kIirC64 = 1, kIirF64 = 2, kIirC128 = 3 };   // the codes of include/skdsp.h (iir_api.hip ties them)
inline bool iir_dbl(int dtype) { return dtype == kIirF64 || dtype == kIirC128; }
inline bool iir_cplx(int dtype) { return dtype == kIirC64 || dtype == kIirC128; }

// the options IIR dispatch reads (struct Options in skdsp_internal.hpp; iir_api.hip fills it)
struct IirRouteOptions { int iir_par = 1, iir_planar = 0, iir_up_fused = 1, iir_dn_full = 0, iir_two_pass = 0, iir_no_mfma = 0; };

enum IirCallKind { kIirFilter, kIirUp, kIirDn, kIirRows };
struct IirCall {
    int kind;
    int64_t n;                   // input samples (per row)
    int rate = 1;                // L of .up, M of .dn
    int64_t nrow = 1, x_stride = 0, y_stride = 0;   // rows
    bool zi = false, zf = false;
    int num_cus = 0;
};

enum IirEngine { kEngSeq, kEngPar, kEngFused, kEngScan, kEngWiden, kEngNarrow, kEngZeroStuff, kEngZeroStuffPlanes, kEngDeinterleave, kEngInterleave,
                 kEngDownsample };
// where a step reads and writes: the caller's x / y (advanced by the row inside a row block), workspace slot 3 (two planes), slot 2 (the
// full-rate result of a .dn that refilters), and the buffers of a handle (`owner`)
enum IirBufKind { kBufX, kBufY, kBufPlanes, kBufFull, kBufGroupTmp, kBufTwinIn, kBufTwinOut };
template <class H> struct IirBuf {
    int kind = kBufX;
    H *owner = nullptr;
    int64_t bytes = 0;           // what the buffer must hold (not the caller's)
    bool operator==(const IirBuf &o) const { return kind == o.kind && owner == o.owner; }
};

template <class H> struct IirStep {
    int engine = kEngScan;
    H *h = nullptr;              // the handle (a group, a twin) whose engine runs
    IirBuf<H> src, dst;
    int64_t n = 0;               // samples per row or plane at the engine's output rate before dec (helpers: input samples / scalars)
    int nrow = 1;                // rows, or 2 planes
    int64_t x_stride = 0, y_stride = 0;
    bool interleaved = false;
    int dec = 1, up = 1;         // helpers: up = L of a zero-stuff, dec = M of a downsample
    bool zi = false, zf = false; // the caller's states: sections [state_first, state_first + h->nsec) of each of its state_D-long vectors
    int state_first = 0, state_D = 0;
    ParChoice par;               // kEngPar
    ScanGeom geom{};             // kEngScan
    bool fast = false;           //   aggregate-free mode
    int block = 0;               // > 0: this and the next block - 1 steps run once per row of the call, rows in order
};

constexpr int kIirNoRoute = -1000;   // no engine takes the call (cannot happen: a planar call is always taken)
template <class H> struct IirRoute {
    int status = 0;              // 0, the negative code a query failed with, or kIirNoRoute
    std::vector<IirStep<H>> steps;
};

template <class H, class Q> struct IirRouter {
    const IirRouteOptions &o;
    Q &q;
    int num_cus;
    IirRoute<H> &r;

    IirStep<H> &push(int engine, H *h, const IirBuf<H> &src, const IirBuf<H> &dst, int64_t n)
    {
        r.steps.emplace_back();
        IirStep<H> &s = r.steps.back();
        s.engine = engine; s.h = h; s.src = src; s.dst = dst; s.n = n;
        return s;
    }
    static int64_t plane_stride(int64_t n) { return (n + 63) / 64 * 64; }
    static IirBuf<H> planes(const H *h, int64_t n) { return IirBuf<H>{kBufPlanes, nullptr, 2 * plane_stride(n) * (iir_dbl(h->dtype) ? 8 : 4)}; }
    struct State { bool zi = false, zf = false; int first = 0, D = 0; };
    // the tables of (h, T), asked once: the interleaved attempt and the planes behind it cut the same chunks
    H *facts_h = nullptr;
    int64_t facts_T = 0;
    ScanFacts facts_f{};
    bool facts(H *h, int64_t T, ScanFacts &f)
    {
        if (facts_h != h || facts_T != T) {
            if ((r.status = q.scan_facts(h, T, facts_f))) return false;
            facts_h = h; facts_T = T;
        }
        f = facts_f;
        return true;
    }

    // One handle over real rows / two planes (nbatch, batch_stride) or, interleaved, over a complex signal.  False: the interleaved form
    // does not take this call (nothing was added; a planar call is always taken) or a query failed (r.status).
    bool planar(H *h, const IirBuf<H> &x, int64_t n, int nbatch, int64_t bs, const IirBuf<H> &y, State st, bool il, int dec, bool par_asked = false)
    {
        const bool dbl = iir_dbl(h->dtype);
        if (st.D == 0) st.D = h->nsec * h->order;
        auto leaf = [&](int engine) -> IirStep<H> & {
            IirStep<H> &s = push(engine, h, x, y, n);
            s.nrow = nbatch; s.x_stride = s.y_stride = bs; s.interleaved = il; s.dec = dec;
            s.zi = st.zi; s.zf = st.zf; s.state_first = st.first; s.state_D = st.D;
            return s;
        };
        if (h->seq) {   // an ill-conditioned cascade: the reference's own recursion (iir_seq.hip)
            if (il) return false;
            leaf(kEngSeq);
            return true;
        }
        if (h->twin64) {   // the float64 detour (see IirHandle::twin64): planar float32 in, planar float32 out
            if (il) return false;
            const int64_t tot = nbatch > 1 ? bs * nbatch : n, out_tot = dec > 1 ? n / dec : tot;
            const IirBuf<H> in{kBufTwinIn, h, tot * 8 + 256};
            const IirBuf<H> o64 = dec > 1 ? IirBuf<H>{kBufTwinOut, h, out_tot * 8 + 256} : in;   // (one real row: the kept outputs go to a buffer of their own)
            push(kEngWiden, h, x, in, tot);
            if (!planar(h->twin64, in, n, nbatch, bs, o64, st, false, dec)) return false;
            push(kEngNarrow, h, o64, y, out_tot);
            return true;
        }
        if (!h->groups.empty()) {
            // consecutive groups of sections: group 0 reads x, the others filter y in place; a decimating call keeps the full-rate signal of all
            // groups but the last in a buffer of the handle; the states are per section, so a group takes its slice
            if (il) return false;
            const IirBuf<H> mid = dec > 1 ? IirBuf<H>{kBufGroupTmp, h, (nbatch > 1 ? bs * nbatch : n) * (dbl ? 8 : 4) + 256} : y;
            for (size_t gi = 0; gi < h->groups.size(); ++gi) {
                H *g = h->groups[gi];
                const bool last = gi + 1 == h->groups.size();
                State sg = st;
                sg.first = g->group_first;
                if (!planar(g, gi == 0 ? x : mid, n, nbatch, bs, last ? y : mid, sg, false, last ? dec : 1)) return false;
            }
            return true;
        }
        // Parallel form (iir_par.hip): the same transfer function as independent two-state branches, every wave its own segment.
        // No state crosses these calls (scipy's zi / zf live in the cascade's coordinates: such calls keep the kernels below).
        // (interleaved complex: re and im are two independent real signals on one memory stream; with dec > 1 only where a segment's kept outputs
        // fit the wave's stage image)
        if (!par_asked && !st.zi && !st.zf && o.iir_par > 0 && h->order == 2 && h->nsec <= 8 && (il || dec <= 1 || nbatch == 1)) {
            const ParChoice c = q.par(h, il, il ? 1 : nbatch, dec, 1, n);
            if (c.status < 0) { r.status = c.status; return false; }
            if (c.status == 0) {
                IirStep<H> &s = leaf(kEngPar);
                s.par = c;
                if (il) { s.nrow = 1; s.x_stride = s.y_stride = 0; }
                return true;
            }
        }
        const int D = h->nsec * h->order;
        int fstate = 0, fnlv = 0;
        if ((r.status = q.fused_cached(h, il, fstate, fnlv))) return false;
        const bool wanted = fused_wanted(h->order, D, o.iir_two_pass, fstate, dec, nbatch, il, st.zf, n, dbl, num_cus);
        if (wanted && fstate == 0) {
            ScanFacts f;
            if (!facts(h, fused_chunk(dbl, il), f)) return false;
            fstate = fused_applies(f, fused_chunk(dbl, il)) ? 1 : -1;
            fnlv = f.n_lv;
            q.fused_remember(h, il, fstate, fnlv);
        }
        if (wanted && fstate == 1 && fused_policy(il, dbl, fnlv, o.iir_two_pass)) {
            leaf(kEngFused);
            return true;
        }
        const ScanGeom g = scan_geometry(n, D);
        ScanFacts f;
        if (!facts(h, g.T, f)) return false;
        const bool fast = scan_fast(f, D, h->order, g.T, o.iir_no_mfma);
        if (il && !scan_interleaved_applies(fast, g.T)) return false;
        IirStep<H> &s = leaf(kEngScan);
        s.geom = g;
        s.fast = fast;
        return true;
    }

    // .filter of a real or interleaved complex vector (y may be x)
    bool filter(H *h, const IirBuf<H> &x, int64_t n, const IirBuf<H> &y, State st, bool par_asked = false)
    {
        if (!iir_cplx(h->dtype)) return planar(h, x, n, 1, 0, y, st, false, 1, par_asked);
        const bool planar_only = o.iir_planar != 0;   // developer A/B switch (and the tests)
        if (!planar_only && !h->groups.empty() && !h->twin64 && !st.zi && !st.zf && o.iir_par > 0) {
            // more than 8 biquads on a complex signal: group after group in place behind the first, each through the parallel form on the
            // interleaved samples where it applies (else whatever that group's own dispatch takes) -- not the whole cascade through two planes
            for (size_t gi = 0; gi < h->groups.size(); ++gi) {
                H *g = h->groups[gi];
                const IirBuf<H> &src = gi == 0 ? x : y;
                const ParChoice c = q.par(g, true, 1, 1, 1, n);
                if (c.status < 0) { r.status = c.status; return false; }
                if (c.status == 0) {
                    IirStep<H> &s = push(kEngPar, g, src, y, n);
                    s.interleaved = true;
                    s.par = c;
                } else if (!filter(g, src, n, y, State(), true)) {
                    return false;
                }
            }
            return true;
        }
        // decaying filters: both components stay interleaved end to end
        if (!planar_only && planar(h, x, n, 2, 0, y, st, true, 1, par_asked)) return true;
        if (r.status) return false;
        return through_planes(h, kEngDeinterleave, x, n, 1, y, st);
    }

    // a complex signal through two real planes: split (or zero-stuff) into workspace slot 3, filter the planes in place, interleave into y
    bool through_planes(H *h, int split, const IirBuf<H> &x, int64_t n_in, int L, const IirBuf<H> &y, State st)
    {
        const int64_t n = n_in * L;
        const IirBuf<H> pl = planes(h, n);
        push(split, h, x, pl, n_in).up = L;
        if (!planar(h, pl, n, 2, plane_stride(n), pl, st, false, 1)) return false;
        push(kEngInterleave, h, pl, y, n);
        return true;
    }

    // y = filter(L * upsample(x, L))
    bool up(H *h, const IirBuf<H> &x, int64_t n, int L, const IirBuf<H> &y)
    {
        const bool cplx = iir_cplx(h->dtype);
        // the parallel-form kernel zero-stuffs while it stages a segment: the L-fold signal is never written
        if (L > 1 && o.iir_par && o.iir_up_fused && h->order == 2 && !(cplx && o.iir_planar)) {
            const ParChoice c = q.par(h, cplx, 1, 1, L, n * L);
            if (c.status < 0) { r.status = c.status; return false; }
            if (c.status == 0) {
                IirStep<H> &s = push(kEngPar, h, x, y, n * L);
                s.interleaved = cplx; s.up = L; s.par = c;
                return true;
            }
        }
        if (cplx) return through_planes(h, kEngZeroStuffPlanes, x, n, L, y, State());
        push(kEngZeroStuff, h, x, y, n).up = L;   // zero-stuff straight into y, then filter in place
        return filter(h, y, n * L, y, State());
    }

    // y = downsample(filter(x), M)
    bool dn(H *h, const IirBuf<H> &x, int64_t n, int M, const IirBuf<H> &y)
    {
        // K3 stores every M-th output itself -- the full-rate result never reaches HBM
        if (M > 1 && M <= 4096 && !o.iir_dn_full) {
            if (!iir_cplx(h->dtype)) return planar(h, x, n, 1, 0, y, State(), false, M);
            if (!o.iir_planar && planar(h, x, n, 2, 0, y, State(), true, M)) return true;   // interleaved complex kernels (decaying filters)
            if (r.status) return false;
        }
        const IirBuf<H> full{kBufFull, nullptr, n * (iir_dbl(h->dtype) ? 8 : 4) * (iir_cplx(h->dtype) ? 2 : 1) + 256};
        if (!filter(h, x, n, full, State())) return false;
        push(kEngDownsample, h, full, y, n).dec = M;
        return true;
    }

    // rows of one launch (parallel form) or, where that does not apply, row by row through the cascade kernels
    bool rows(H *h, const IirCall &c, const IirBuf<H> &x, const IirBuf<H> &y)
    {
        const bool real = !iir_cplx(h->dtype);
        auto par_rows = [&](H *g, const IirBuf<H> &src, int64_t ss) -> int {   // 0: added, 1: not taken, < 0: r.status
            const ParChoice pc = q.par(g, false, (int)c.nrow, 1, 1, c.n);
            if (pc.status == 0) {
                IirStep<H> &s = push(kEngPar, g, src, y, c.n);
                s.nrow = (int)c.nrow; s.x_stride = ss; s.y_stride = c.y_stride; s.par = pc;
            }
            if (pc.status < 0) r.status = pc.status;
            return pc.status;
        };
        auto row_by_row = [&](H *g, const IirBuf<H> &src, bool par_asked) -> bool {
            const size_t first = r.steps.size();
            if (!filter(g, src, c.n, y, State(), par_asked)) return false;
            r.steps[first].block = (int)(r.steps.size() - first);
            return true;
        };
        // the reference's recursion takes all rows in ONE launch (one wave per row), not one single-wave kernel per row in stream order
        if (h->seq && real) {
            IirStep<H> &s = push(kEngSeq, h, x, y, c.n);
            s.nrow = (int)c.nrow; s.x_stride = c.x_stride; s.y_stride = c.y_stride;
            return true;
        }
        if (!h->groups.empty() && real && o.iir_par > 0) {
            // groups of sections (more than 8 biquads): every group over all rows in one launch where its parallel form applies, in place behind the first
            for (size_t gi = 0; gi < h->groups.size(); ++gi) {
                const IirBuf<H> &src = gi == 0 ? x : y;
                const int took = par_rows(h->groups[gi], src, gi == 0 ? c.x_stride : c.y_stride);
                if (took < 0 || (took > 0 && !row_by_row(h->groups[gi], src, c.nrow == 1))) return false;
            }
            return true;
        }
        bool asked = false;
        if (real && o.iir_par > 0) {
            const int took = par_rows(h, x, c.x_stride);
            if (took <= 0) return took == 0;
            asked = c.nrow == 1;   // (the same question: one real row)
        }
        return row_by_row(h, x, asked);
    }
};

// the route of one call (n > 0 and, for rows, nrow > 0: the entry points answer the empty calls themselves)
template <class H, class Q> inline IirRoute<H> iir_route(H *h, const IirCall &c, const IirRouteOptions &o, Q &q)
{
    IirRoute<H> r;
    IirRouter<H, Q> w{o, q, c.num_cus, r};   // (aggregate: the memo members take their defaults)
    const IirBuf<H> x{kBufX, nullptr, 0}, y{kBufY, nullptr, 0};
    typename IirRouter<H, Q>::State st;
    st.zi = c.zi; st.zf = c.zf;
    bool ok;
    if (c.kind == kIirUp) ok = w.up(h, x, c.n, c.rate, y);
    else if (c.kind == kIirDn) ok = w.dn(h, x, c.n, c.rate, y);
    else if (c.kind == kIirRows) ok = w.rows(h, c, x, y);
    else ok = w.filter(h, x, c.n, y, st);
    if (!ok && r.status == 0) r.status = kIirNoRoute;
    return r;
}

}  // namespace skdsp
