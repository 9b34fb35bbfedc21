// timing_core.hpp -- the recipe, the plans and the per-thread functions of non-data-aided symbol timing recovery over a frame set,
// synchronization.NDA_symb_sync (synchronization.py:43-166 of the reference).  Plain C++ for host and device: timing.hip builds its kernels from it
// and tests/host/nda_emul.cpp walks the same functions thread by thread without a GPU.
//
// The loop.  A row is a frame from rest; zp is the row with one zero sample in front (zp[0] = 0, zp[i] = x[row, start + i - 1]).  Iteration
// nn = 1 ... N - 1, N = Ns (floor((n + 1) / Ns) - (Ns - 1)), in the reference's order:
//   CNT = CNT_next, mu = mu_next
//   if the last iteration underflowed (the HEAVY step, once per symbol):
//       Ns Farrow interpolants at nn + kk, kk = 0 ... Ns - 1, of order 1, 2 or 3 from zp[nn + kk - 1 ... nn + kk + 2]; the one at kk = 0 is z_interp (the
//       reference computes it twice, from the same operands in the same order).  Per component, since every coefficient and mu are real:
//           order 1:  mu z[nn] + (1 - mu) z[nn - 1]
//           order 2:  v2 = 0.5 S(1, -1, -1, 1), v1 = 0.5 S(-1, 3, -1, -1), v0 = z[nn];   (mu v2 + v1) mu + v0
//           order 3:  v3 = S(1/6., -1/2., 1/2., -1/6.), v2 = S(0, 1/2., -1, 1/2.), v1 = S(-1/6., 1, -1/2., -1/3.);   ((mu v3 + v2) mu + v1) mu + v0
//       S(c0, c1, c2, c3) = np.sum of the products t0 = z[nn + 2] c0, t1 = z[nn + 1] c1, t2 = z[nn] c2, t3 = z[nn - 1] c3, which NumPy adds as
//       (t0 + t1) + (t2 + t3) (tests/golden/g28_conventions.json: its complex sum keeps four accumulators from four elements on).
//       c1 = (sum over kk of |interp|^2 rot[kk]) (1 / Ns): |.|^2 is re re + im im (the reference squares hypot: a documented departure), rot[kk] the
//       host's np.exp(-1j 2 pi / Ns kk), the sum from 0 in kk order, the quotient NumPy's product with the reciprocal.
//       The 2L + 1 buffer takes c1 in front; epsilon = (-1 / (2 pi)) atan2_rn(im q, re q), q = np.sum(buffer) (1 / (2L + 1)), the sum RE-FORMED at
//       every symbol in NumPy's order for that length (np_csum below).  zz[mm] = z_interp, e_tau[mm] = epsilon, mm += 1.
//   vp = K1 epsilon, vi += K2 epsilon (on every sample: epsilon holds its value while the loop coasts), W = 1 / Ns + (vp + vi)
//   CNT_next = CNT - W; below zero: CNT_next = 1 + CNT_next, underflow, mu_next = CNT / W (a true division); else mu_next = mu
// The outputs are zz[:mm - 1], e_tau[:mm - 1]: index 0 is 0 and the last stored symbol is dropped, so a symbol is stored when the NEXT one is made
// (`pending` below) and counts[row] = mm - 1.  Float64 throughout, never contracted; complex64 is storage (widened at the load, zz rounded once at
// the store).  A NaN never underflows, so a non-finite sample reaches epsilon through |.|^2 and holds the row's counter for good.
//
// Geometry.  One wave64 per workgroup serves 64 rows, a lane per row.  A tile is 64 rows x kTile iterations and carries zp[tile kTile ... tile kTile
// + kTile + Ns + 1] per row: one sample behind the first iteration and Ns + 1 ahead of the last.  The wave loads it as runs along the rows, keeps
// it in registers while the previous tile is walked, and puts it into LDS with an odd row pitch.  The walk is symbol-major: a lane coasts, in cheap
// per-sample steps, to its own next underflow; the heavy step is the code behind that loop, where the lanes of the wave meet again and take it
// together.  The 2L + 1 buffer is a ring per lane in LDS: L is a run-time value, and a register array indexed by it would live in scratch memory.
// Outputs leave the walk as plain stores, one element per lane and symbol.
//
// The scale.  zz /= np.std(zz) is a second kernel, one workgroup of kNormThreads per row over min(counts[row], cap) elements: np.std's two passes
// (the mean, then the mean squared distance from it) with each sum formed as kNormThreads strided partial sums and a fixed tree over them, then
// zz (1 / std) per component, which is how NumPy divides a complex array by a float64 scalar.  No atomics: two runs give the same bits.
#pragma once
#include "carrier_core.hpp"

namespace skdsp {
namespace tim {

constexpr int kLane = 64;                        // rows of a workgroup: one wave64, a lane per row
constexpr int kTile = 16;                        // loop iterations of a tile
constexpr int kMinNs = 2, kMaxNs = 16, kMaxL = 8;
constexpr int kMaxW = kTile + kMaxNs + 2;        // samples of a tile's row at most (and elements a lane moves per tile)
constexpr int kNormThreads = 256;
constexpr int64_t kMaxLen = (int64_t)1 << 40;
enum Out { kOutZ = 1, kOutE = 2, kOutAll = 3 };

// ------------------------------------------------------------------------------------------------------------------ the recipe
// np.sum of n complex values in NumPy's order: below four elements left to right; from four on, accumulator k takes elements k, k + 4, ... of the
// leading multiple of four, the four merge as (r0 + r1) + (r2 + r3), and the remaining elements follow one by one.  get(i, &re, &im).
template <class F> SK_HD void np_csum(int n, F get, double *sr, double *si)
{
    SK_NO_CONTRACT
    double xr, xi;
    if (n < 4) {
        get(0, sr, si);
        for (int i = 1; i < n; ++i) {
            get(i, &xr, &xi);
            *sr = *sr + xr;
            *si = *si + xi;
        }
        return;
    }
    double rr[4], ri[4];
    for (int k = 0; k < 4; ++k) get(k, &rr[k], &ri[k]);
    int i = 4;
    for (; i < n - (n % 4); i += 4)
        for (int k = 0; k < 4; ++k) {
            get(i + k, &xr, &xi);
            rr[k] = rr[k] + xr;
            ri[k] = ri[k] + xi;
        }
    *sr = (rr[0] + rr[1]) + (rr[2] + rr[3]);
    *si = (ri[0] + ri[1]) + (ri[2] + ri[3]);
    for (; i < n; ++i) {
        get(i, &xr, &xi);
        *sr = *sr + xr;
        *si = *si + xi;
    }
}

// S(c0, c1, c2, c3) of one component: a0 ... a3 = z[nn - 1], z[nn], z[nn + 1], z[nn + 2]
SK_HD double farrow_sum(double a0, double a1, double a2, double a3, double c0, double c1, double c2, double c3)
{
    SK_NO_CONTRACT
    const double t0 = a3 * c0, t1 = a2 * c1, t2 = a1 * c2, t3 = a0 * c3;
    return (t0 + t1) + (t2 + t3);
}
// one component of the interpolant of order IORD at fractional interval mu
template <int IORD> SK_HD double interp(double mu, double a0, double a1, double a2, double a3)
{
    SK_NO_CONTRACT
    if (IORD == 1) {
        const double p = mu * a1, om = 1.0 - mu;
        return p + om * a0;
    }
    if (IORD == 2) {
        const double v2 = 0.5 * farrow_sum(a0, a1, a2, a3, 1.0, -1.0, -1.0, 1.0), v1 = 0.5 * farrow_sum(a0, a1, a2, a3, -1.0, 3.0, -1.0, -1.0);
        return (mu * v2 + v1) * mu + a1;
    }
    const double v3 = farrow_sum(a0, a1, a2, a3, 1 / 6., -1 / 2., 1 / 2., -1 / 6.), v2 = farrow_sum(a0, a1, a2, a3, 0.0, 1 / 2., -1.0, 1 / 2.);
    const double v1 = farrow_sum(a0, a1, a2, a3, -1 / 6., 1.0, -1 / 2., -1 / 3.);
    return ((mu * v3 + v2) * mu + v1) * mu + a1;
}

struct Loop {                      // what a call fixes for every row
    int ns = 4, len = 1;           // samples per symbol; 2L + 1
    double inv_ns = 0.25, inv_len = 1.0, k_eps = 0.0;    // the host's 1 / float(Ns), 1.0 / (2L + 1), -1 / (2 np.pi)
    const double *rot_re = nullptr, *rot_im = nullptr;   // the host's np.exp(-1j 2 np.pi / Ns kk), Ns entries (the kernel: a copy in LDS)
};
struct Row {
    double k1, k2;
};
struct State {
    double cnt, mu, eps, vi;       // CNT_next, mu_next, epsilon, the integrator
    double pr, pi, pe;             // the symbol made last, stored when the next one is made
    int64_t mm;                    // the reference's mm
    int under, head;               // the underflow flag; where the newest entry of the ring lies
};
SK_HD State state_rest() { return State{0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1, 0, 0}; }

// the loop filter and the counter of one iteration: what every sample takes, coasting or not
SK_HD void counter_step(const Loop &lp, const Row &w, State &st)
{
    SK_NO_CONTRACT
    const double cnt = st.cnt;
    const double vp = w.k1 * st.eps;
    st.vi = st.vi + w.k2 * st.eps;
    const double v = vp + st.vi;
    const double W = lp.inv_ns + v;
    const double next = cnt - W;
    if (next < 0.0) {
        st.cnt = 1.0 + next;
        st.under = 1;
        st.mu = cnt / W;
    } else {
        st.cnt = next;
        st.under = 0;
    }
}

// The heavy step at the iteration whose zp[nn - 1] lies at complex slot `at` of the lane's LDS row: the interpolants, c1 into the ring at
// `ring` (complex slots, lp.len of them), epsilon.  z_interp leaves in (zr, zi).  Lds: ld2 / st2.
template <int IORD, class Lds> SK_HD void heavy_step(const Loop &lp, State &st, int at, int ring, const Lds &L, double *zr, double *zi)
{
    SK_NO_CONTRACT
    const double mu = st.mu;
    double ar[4], ai[4];
    ar[3] = ai[3] = 0.0;
    L.ld2(2 * at, &ar[0], &ai[0]);
    L.ld2(2 * (at + 1), &ar[1], &ai[1]);
    if (IORD > 1) L.ld2(2 * (at + 2), &ar[2], &ai[2]);
    else ar[2] = ai[2] = 0.0;
    double cr = 0.0, ci = 0.0;
    for (int kk = 0; kk < lp.ns; ++kk) {
        if (IORD > 1) L.ld2(2 * (at + kk + 3), &ar[3], &ai[3]);
        const double ir = interp<IORD>(mu, ar[0], ar[1], ar[2], ar[3]), ii = interp<IORD>(mu, ai[0], ai[1], ai[2], ai[3]);
        if (kk == 0) {
            *zr = ir;
            *zi = ii;
        }
        const double m2 = ir * ir + ii * ii;
        cr = cr + m2 * lp.rot_re[kk];
        ci = ci + m2 * lp.rot_im[kk];
        ar[0] = ar[1], ai[0] = ai[1];
        if (IORD > 1) {
            ar[1] = ar[2], ai[1] = ai[2];
            ar[2] = ar[3], ai[2] = ai[3];
        } else if (kk + 1 < lp.ns)
            L.ld2(2 * (at + kk + 2), &ar[1], &ai[1]);
    }
    cr = cr * lp.inv_ns;
    ci = ci * lp.inv_ns;
    st.head = (st.head == 0 ? lp.len : st.head) - 1;
    L.st2(2 * (ring + st.head), cr, ci);
    double sr, si;
    const int head = st.head, len = lp.len;
    np_csum(len, [&](int i, double *re, double *im) {
        const int k = head + i;
        L.ld2(2 * (ring + (k >= len ? k - len : k)), re, im);
    }, &sr, &si);
    sr = sr * lp.inv_len;
    si = si * lp.inv_len;
    st.eps = lp.k_eps * sym::atan2_rn(si, sr);
}

// ------------------------------------------------------------------------------------------------------------------ the plan
// N of the reference for a frame of n samples: the loop runs nn = 1 ... N - 1
SK_HD int64_t loop_end(int64_t n, int ns)
{
    const int64_t N = (int64_t)ns * ((n + 1) / ns - (ns - 1));
    return N > 0 ? N : 0;
}
SK_HD int64_t loop_iters(int64_t n, int ns)
{
    const int64_t N = loop_end(n, ns);
    return N > 1 ? N - 1 : 0;
}

struct Plan {
    int ns = 4, L = 0, iord = 3, c64 = 0, z64 = 0, outs = kOutAll;   // c64: complex64 samples; z64: zz leaves as complex64 (else complex128)
    int W = 0, pitch = 0, at_ring = 0, lds_doubles = 0;              // samples and complex slots of a tile's row; the rings; the LDS image in doubles
    int64_t n = 0, nrow = 0, start = 0, x_stride = 0, y_stride = 0, z_stride = 0, cap = 0, iters = 0, tiles = 0, groups = 0;   // z_stride: zz's rows (y_stride unless the launch redirects zz)
};
inline const char *plan_make(int ns, int L, int iord, int dtype, int z64, int outs, int64_t n, int64_t nrow, int64_t start, int64_t x_stride, int64_t y_stride, int64_t cap, Plan *p)
{
    if (ns < kMinNs || ns > kMaxNs) return "Ns must be an integer in 2 ... 16";
    if (L < 0 || L > kMaxL) return "L must be an integer in 0 ... 8";
    if (iord < 1 || iord > 3) return "I_ord must be 1, 2 or 3";
    if (dtype != 1 && dtype != 3) return "complex64 or complex128 samples";
    if (outs < 1 || outs > kOutAll) return "at least one of zz, e_tau";
    if (n < 0 || nrow < 0 || n >= kMaxLen || nrow >= kMaxLen) return "need 0 <= n, nrow < 2^40";
    if (start < 0 || start >= kMaxLen || cap < 0 || cap >= kMaxLen) return "need 0 <= start, cap < 2^40";
    if (x_stride < 0 || y_stride < cap || x_stride >= kMaxLen || y_stride >= kMaxLen) return "need 0 <= x_stride and cap <= y_stride, both below 2^40";
    if (n > 0 && x_stride < start + n) return "x_stride is smaller than the window a row is read from";
    const int64_t N = loop_end(n, ns);
    if (N > 1 && iord > 1 && N + ns > n) return "for Ns = 2 with I_ord >= 2 a frame of odd length makes the reference's slices run past its array";
    if (z64 && dtype != 1) return "complex64 symbols come from complex64 samples";
    p->ns = ns;
    p->L = L;
    p->iord = iord;
    p->c64 = dtype == 1;
    p->z64 = z64 ? 1 : 0;
    p->outs = outs;
    p->W = kTile + ns + 2;
    p->pitch = p->W | 1;
    p->at_ring = 2 * kLane * p->pitch;
    p->lds_doubles = p->at_ring + 2 * kLane * (2 * L + 1);
    p->n = n;
    p->nrow = nrow;
    p->start = start;
    p->x_stride = x_stride;
    p->y_stride = y_stride;
    p->z_stride = y_stride;
    p->cap = cap;
    p->iters = loop_iters(n, ns);
    p->tiles = (p->iters + kTile - 1) / kTile;
    p->groups = (nrow + kLane - 1) / kLane;
    if (p->groups > (((int64_t)1 << 31) - 1)) return "too many rows for one launch";
    return nullptr;
}
SK_HD int tile_count(const Plan &p, int64_t tile)
{
    const int64_t left = p.iters - tile * kTile;
    return left < kTile ? (int)left : kTile;
}

// (C64 of the movers below: the plan's c64, a compile-time constant, as in carrier_core.hpp)
// Lane t's share of a tile's loads, into registers: element e = j 64 + t is row e / W of the group, slot e mod W of the tile.  Slot s holds
// zp[tile kTile + s]; zp[0], what lies behind the frame and what no iteration of the tile reads stay zero and are not loaded.
template <bool C64, class Mem> SK_HD void tile_fetch(const Mem &m, const Plan &p, const void *x, int64_t group, int64_t tile, int t, car::Sample *regs)
{
    const int need = tile_count(p, tile) + p.ns + 2;
    const int q = kLane / p.W, rm = kLane % p.W;
    int rl = t / p.W, s = t % p.W;
    SK_UNROLL
    for (int j = 0; j < kMaxW; ++j) {
        regs[j].re = regs[j].im = 0.0;
        if (j < p.W) {
            const int64_t row = group * kLane + rl, i = tile * kTile + s;
            if (row < p.nrow && s < need && i >= 1 && i <= p.n) {
                const int64_t at = row * p.x_stride + p.start + i - 1;
                if (C64) regs[j].re = chan::bits_to_double(m.ld_u64(static_cast<const float *>(x) + 2 * at));
                else m.ld_c128(static_cast<const double *>(x) + 2 * at, &regs[j].re, &regs[j].im);
            }
            rl += q;
            s += rm;
            if (s >= p.W) {
                s -= p.W;
                rl += 1;
            }
        }
    }
}
// the registers into the LDS image, every slot of the tile
template <bool C64, class Lds> SK_HD void tile_put(const Plan &p, int t, const car::Sample *regs, const Lds &L)
{
    const int q = kLane / p.W, rm = kLane % p.W;
    int rl = t / p.W, s = t % p.W;
    SK_UNROLL
    for (int j = 0; j < kMaxW; ++j) {
        if (j < p.W) {
            double re = regs[j].re, im = regs[j].im;
            if (C64) {
                const uint64_t bits = chan::double_to_bits(re);
                const uint32_t lo = (uint32_t)bits, hi = (uint32_t)(bits >> 32);
                float fr, fi;
                memcpy(&fr, &lo, 4);
                memcpy(&fi, &hi, 4);
                re = (double)fr;
                im = (double)fi;
            }
            L.st2(2 * (rl * p.pitch + s), re, im);
            rl += q;
            s += rm;
            if (s >= p.W) {
                s -= p.W;
                rl += 1;
            }
        }
    }
}
// the lane's ring starts as the reference's np.zeros(2L + 1)
template <class Lds> SK_HD void ring_clear(const Plan &p, int t, const Lds &L)
{
    for (int i = 0; i < 2 * p.L + 1; ++i) L.st2(p.at_ring + 2 * (t * (2 * p.L + 1) + i), 0.0, 0.0);
}
// the symbol made last goes to index mm - 1 of the row (index 0: the zeros the state starts with), unless the row has outgrown cap
template <class Mem> SK_HD void pending_store(const Mem &m, const Plan &p, void *z, double *e, int64_t row, const State &st)
{
    const int64_t j = st.mm - 1;
    if (j >= p.cap) return;
    if (p.outs & kOutZ) {
        const int64_t at = row * p.z_stride + j;
        if (p.z64) m.st_c64(static_cast<float *>(z) + 2 * at, (float)st.pr, (float)st.pi);
        else m.st_c128(static_cast<double *>(z) + 2 * at, st.pr, st.pi);
    }
    if (p.outs & kOutE) m.st_f64(e + row * p.y_stride + j, st.pe);
}
// Lane t walks its row through the tile, symbol-major: coast to the next underflow, then the heavy step.  On the GPU the lanes of the wave leave
// the coasting loop one by one and take what follows it together.
template <int IORD, class Mem, class Lds> SK_HD void tile_walk(const Mem &m, const Plan &p, const Loop &lp, const Row &w, int64_t group, int64_t tile, int t, State &st, const Lds &L, void *z, double *e)
{
    const int64_t row = group * kLane + t;
    if (row >= p.nrow) return;
    const int cnt = tile_count(p, tile);
    const int base = t * p.pitch, ring = p.at_ring / 2 + t * lp.len;
    int pos = 0;
    while (pos < cnt) {
        while (pos < cnt && !st.under) {
            counter_step(lp, w, st);
            ++pos;
        }
        if (pos < cnt) {
            double zr, zi;
            heavy_step<IORD>(lp, st, base + pos, ring, L, &zr, &zi);
            pending_store(m, p, z, e, row, st);
            st.pr = zr;
            st.pi = zi;
            st.pe = st.eps;
            st.mm += 1;
            counter_step(lp, w, st);
            ++pos;
        }
    }
}
template <class Mem> SK_HD Row row_of(const Mem &m, double k1, double k2, const double *gains, int64_t row, int64_t nrow)
{
    Row w = {k1, k2};
    if (gains && row < nrow) {
        w.k1 = m.ld_f64(gains + 2 * row);
        w.k2 = m.ld_f64(gains + 2 * row + 1);
    }
    return w;
}

// ------------------------------------------------------------------------------------------------------------------ the scale
// Thread t of kNormThreads, row `row`, n = min(counts[row], cap) elements of complex128 at raw + 2 row raw_stride.  Slots: 2 kNormThreads doubles.
// Phases, a barrier behind each:  norm_sums -> norm_tree(off = kNormThreads / 2 ... 1) -> norm_dists (reads slot 0) -> norm_tree(...) -> norm_store
struct NormPlan {
    int z64 = 0;
    int64_t nrow = 0, cap = 0, raw_stride = 0, y_stride = 0;
};
inline const char *norm_plan_make(int z64, int64_t nrow, int64_t cap, int64_t raw_stride, int64_t y_stride, NormPlan *p)
{
    if (nrow < 0 || cap < 0 || nrow >= (((int64_t)1 << 31) - 1) || cap >= kMaxLen) return "need 0 <= nrow < 2^31 - 1 and 0 <= cap < 2^40";
    if (raw_stride < cap || y_stride < cap || raw_stride >= kMaxLen || y_stride >= kMaxLen) return "need cap <= raw_stride, y_stride < 2^40";
    p->z64 = z64 ? 1 : 0;
    p->nrow = nrow;
    p->cap = cap;
    p->raw_stride = raw_stride;
    p->y_stride = y_stride;
    return nullptr;
}
template <class Mem> SK_HD int64_t norm_len(const Mem &m, const NormPlan &p, const int64_t *counts, int64_t row)
{
    const int64_t c = (int64_t)m.ld_u64(counts + row);
    return c < 0 ? 0 : c < p.cap ? c : p.cap;
}
template <class Mem, class Lds> SK_HD void norm_sums(const Mem &m, const NormPlan &p, const double *raw, int64_t row, int64_t n, int t, const Lds &S)
{
    SK_NO_CONTRACT
    double sr = 0.0, si = 0.0;
    for (int64_t j = t; j < n; j += kNormThreads) {
        double re, im;
        m.ld_c128(raw + 2 * (row * p.raw_stride + j), &re, &im);
        sr = sr + re;
        si = si + im;
    }
    S.st2(2 * t, sr, si);
}
template <class Lds> SK_HD void norm_tree(int off, int t, const Lds &S)
{
    SK_NO_CONTRACT
    if (t >= off) return;
    double ar, ai, br, bi;
    S.ld2(2 * t, &ar, &ai);
    S.ld2(2 * (t + off), &br, &bi);
    S.st2(2 * t, ar + br, ai + bi);
}
// (mr, mi): the mean, read by every thread from slot 0 in front of the barrier that precedes this phase's stores
template <class Mem, class Lds> SK_HD void norm_dists(const Mem &m, const NormPlan &p, const double *raw, int64_t row, int64_t n, int t, double mr, double mi, const Lds &S)
{
    SK_NO_CONTRACT
    double q = 0.0;
    for (int64_t j = t; j < n; j += kNormThreads) {
        double re, im;
        m.ld_c128(raw + 2 * (row * p.raw_stride + j), &re, &im);
        const double dr = re - mr, di = im - mi;
        q = q + (dr * dr + di * di);
    }
    S.st2(2 * t, q, 0.0);
}
// rcp = 1.0 / sqrt(Q / n)
template <class Mem> SK_HD void norm_store(const Mem &m, const NormPlan &p, const double *raw, void *y, int64_t row, int64_t n, int t, double rcp)
{
    SK_NO_CONTRACT
    for (int64_t j = t; j < n; j += kNormThreads) {
        double re, im;
        m.ld_c128(raw + 2 * (row * p.raw_stride + j), &re, &im);
        re = re * rcp;
        im = im * rcp;
        const int64_t at = row * p.y_stride + j;
        if (p.z64) m.st_c64(static_cast<float *>(y) + 2 * at, (float)re, (float)im);
        else m.st_c128(static_cast<double *>(y) + 2 * at, re, im);
    }
}

}  // namespace tim
}  // namespace skdsp
