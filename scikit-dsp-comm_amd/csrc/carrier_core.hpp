// carrier_core.hpp -- the step, the plans and the per-thread functions of decision-directed carrier phase tracking over a frame set,
// synchronization.DD_carrier_sync (synchronization.py:169-275 of the reference), and of the two impairment helpers phase_step / time_step
// (:278-313).  Plain C++ for host and device: carrier.hip builds its kernels from it and tests/host/carrier_emul.cpp walks the same functions
// thread by thread without a GPU.
//
// The loop.  A row is a frame from rest (theta_hat = 0, vi = 0); symbol k of a row is x[row, start + k step].  Per symbol, in the reference's order:
//   z' = z exp(-1j theta_hat)       (c, s) = sincos_rad(theta_hat); re = a c - b d, im = a d + b c with d = -s: four products, two sums
//   a_hat = decision(z')            MPSK 2: sign(re);  MPSK 4: (sign(re), sign(im)) (1 / sqrt 2) -- NumPy's complex quotient by a real is a product
//                                   with the reciprocal;  MPSK > 4: the host's table exp(1j 2 pi a / M) at a = mod(rint(angle(z') M / 2 / pi), M);
//                                   MQAM: 2 clip(rint((z' + x_m (1 + 1j)) / 2), 0, x_m) - x_m (1 + 1j) per component, ties to even.  sign(0) = 0.
//   e_phi                           type 0: im(z') re(a) - re(z') im(a);  type 1: angle(exp(1j (angle(z') - angle(a))));  type 2: im(z' / a), NumPy's
//                                   complex division (Smith's: a zero decision gives im(z') / 0)
//   vi += K2 e; theta_hat = np.mod(theta_hat + (K1 e + vi), 2 pi): the EXACT remainder (fmod), plus 2 pi when it is negative; a zero remainder is +0
//   theta_h = theta_hat, logged behind the wrap; open_loop then sets theta_hat = 0
// MQAM rows are scaled first, z r with r = 1 / (np.std(row) sqrt(3 / (2 (M - 1)))) per component (symmap_core.hpp's deterministic moment merge wrote
// r), and z' leaves multiplied by 1 / r.  Float64 throughout, never contracted: _ffi.carrier_step_host restates every operation in NumPy and gets the
// same bits.  complex64 is a storage type: widened exactly at the load, z' and a_hat rounded once at the store.
//
// sincos_rad.  |x| <= 8 radians: k = the nearest multiple of pi / 2, x - k pi / 2 by Cody and Waite's three-word split (k P1, k P2 exact), kept as a
// head and a tail, the polynomial stage of channel_core.hpp on the head's magnitude, the tail through the derivative.  + - * / only.
//
// Geometry.  One wave64 per workgroup serves 64 rows, a lane per row: a row's symbols are a serial chain.  A tile is 64 rows x kTile symbols.  The
// wave loads it as runs along the rows (element e = j 64 + t of the tile is row e / kTile, symbol e mod kTile: 8 consecutive lanes, 8 consecutive
// symbols), keeps it in registers while the previous tile is walked, and puts it into LDS with a row pitch of kTile + 1 elements: the lanes of the
// walk, a pitch apart, meet no bank twice.  The walk writes the selected outputs back to LDS (z' over the sample it was made from), and the wave
// stores them as the same runs.  Only the selected outputs take LDS and stores.
#pragma once
#include "symmap_core.hpp"
#include "channel_core.hpp"

namespace skdsp {
namespace car {

constexpr int kLane = 64;                       // rows of a workgroup: one wave64, a lane per row
constexpr int kTile = 8;                        // symbols of a tile
constexpr int kPitch = kTile + 1;               // elements from row to row in LDS
constexpr int kPer = kTile;                     // elements a lane moves per tile (64 rows x kTile symbols / 64 lanes)
constexpr int64_t kMaxLen = (int64_t)1 << 40;
enum Out { kOutZ = 1, kOutA = 2, kOutE = 4, kOutT = 8, kOutAll = 15 };

// ------------------------------------------------------------------------------------------------------------------ sincos of radians
// sin and cos of x, |x| <= 8 (anything else, a NaN included: NaN for both)
SK_HD void sincos_rad(double x, double *s, double *c)
{
    SK_NO_CONTRACT
    const double ax = x < 0.0 ? -x : x;
    if (!(ax <= 8.0)) {
        *s = *c = (x - x) / (x - x);
        return;
    }
    const int k = (int)(ax * 0x1.45f306dc9c883p-1 + 0.5);       // the nearest multiple of pi / 2 (0 ... 5); where x is half way, either side serves
    const double dk = (double)k;
    const double t1 = ax - dk * 0x1.921fb54442d10p+0;            // exact: k P1 has 53 bits at most, and the difference fits
    const double p2 = dk * 0x1.08d313198a2e0p-49;                // exact
    const double h0 = t1 - p2, bb = h0 - t1;                     // two_sum(t1, -p2)
    const double l0 = (t1 - (h0 - bb)) + (-p2 - bb);
    const double l1 = l0 - dk * 0x1.b839a252049c1p-104;
    const double h = h0 + l1, l = l1 - (h - h0);                 // |h| <= pi / 4 (+ an ulp), l its tail
    const double ah = h < 0.0 ? -h : h;
    double sh, ch;
    chan::sincos_octant(ah, &sh, &ch);
    if (h < 0.0) sh = -sh;
    const double sr = sh + l * ch, cr = ch - l * sh;            // sin(h + l), cos(h + l)
    const int q = k & 3;
    double sa = (q & 1) ? cr : sr, ca = (q & 1) ? sr : cr;
    if (q & 2) sa = -sa;
    if (q == 1 || q == 2) ca = -ca;
    *s = x < 0.0 ? -sa : sa;
    *c = ca;
}

// np.mod(a, 2 pi) as NumPy computes it (npy_divmod): the exact remainder, the divisor's sign
SK_HD double wrap_2pi(double a)
{
    SK_NO_CONTRACT
    const double two_pi = 0x1.921fb54442d18p+2;
    double m;                                     // below 4 pi in magnitude the remainder is a itself or one exact sum (Sterbenz): fmod's value, without its loop
    if (a > -two_pi && a < two_pi) m = a;
    else if (a >= two_pi && a < 2.0 * two_pi) m = a - two_pi;
    else if (a <= -two_pi && a > -2.0 * two_pi) m = a + two_pi;
    else m = fmod(a, two_pi);
    if (m != 0.0) {
        if (m < 0.0) m = m + two_pi;
    } else {
        m = 0.0;                                  // (a NaN took the branch above and stays)
    }
    return m;
}

// np.sign: 0 for a zero of either sign, NaN for NaN
SK_HD double sign_np(double v) { return v > 0.0 ? 1.0 : v < 0.0 ? -1.0 : v == v ? 0.0 : v; }

// imag((ar + 1j ai) / (br + 1j bi)) as NumPy's complex division computes it
SK_HD double cdiv_imag_np(double ar, double ai, double br, double bi)
{
    SK_NO_CONTRACT
    const double abr = fabs(br), abi = fabs(bi);
    if (abr >= abi) {
        if (abr == 0.0 && abi == 0.0) return ai / abr;
        const double rat = bi / br, scl = 1.0 / (br + bi * rat);
        return (ai - ar * rat) * scl;
    }
    const double rat = br / bi, scl = 1.0 / (bi + br * rat);
    return (ai * rat - ar) * scl;
}

// ------------------------------------------------------------------------------------------------------------------ the step
struct Loop {                      // what a call fixes for every row
    int mod = 2, x_m = 1, open_loop = 0;
    double inv_sqrt2 = 0.0;        // the host's 1.0 / np.sqrt(2) (MPSK 4)
    const double *tab_re = nullptr, *tab_im = nullptr;   // MPSK > 4: the host's np.exp(1j 2 pi a / M), `mod` entries (the kernel: a copy in LDS)
};
struct Row {                       // what a row fixes: the gains, the scale and its reciprocal (1, 1 for MPSK)
    double k1, k2, r, back;
};
struct State {
    double theta, vi;
};
struct StepOut {
    double zr, zi, ar, ai, e, th;
};

// FAM: sym::kQam / sym::kMpsk; TYPE: 0, 1, 2.  (xr, xi): the sample, widened.  zr, zi leave BEFORE the MQAM factor `back` (the store applies it).
template <int FAM, int TYPE> SK_HD void step(const Loop &p, const Row &w, State &st, double xr, double xi, StepOut &o)
{
    SK_NO_CONTRACT
    if (FAM == sym::kQam) {
        xr = xr * w.r;
        xi = xi * w.r;
    }
    double s, c;
    sincos_rad(st.theta, &s, &c);
    const double d = -s;
    const double zr = xr * c - xi * d, zi = xr * d + xi * c;
    double ar, ai;
    if (FAM == sym::kMpsk) {
        if (p.mod == 2) {
            ar = sign_np(zr) + 0.0;
            ai = 0.0;
        } else if (p.mod == 4) {
            ar = sign_np(zr) * p.inv_sqrt2;
            ai = sign_np(zi) * p.inv_sqrt2;
        } else {
            sym::DemapPlan dp;
            dp.kind = sym::kMpsk;
            dp.mod = p.mod;
            const int idx = sym::mpsk_index(zr, zi, dp);
            ar = p.tab_re[idx];
            ai = p.tab_im[idx];
        }
    } else {
        const int kI = sym::qam_level(zr, 1.0, p.x_m), kQ = sym::qam_level(zi, 1.0, p.x_m);
        ar = (double)(2 * kI - p.x_m);
        ai = (double)(2 * kQ - p.x_m);
    }
    double e;
    if (TYPE == 0) {
        const double p1 = zi * ar, p2 = zr * ai;
        e = p1 - p2;
    } else if (TYPE == 1) {
        const double e0 = sym::atan2_rn(zi, zr) - sym::atan2_rn(ai, ar);
        double se, ce;
        sincos_rad(e0, &se, &ce);
        e = sym::atan2_rn(se, ce);
    } else {
        e = cdiv_imag_np(zr, zi, ar, ai);
    }
    const double vp = w.k1 * e;
    st.vi = st.vi + w.k2 * e;
    const double v = vp + st.vi;
    st.theta = wrap_2pi(st.theta + v);
    o.zr = zr;
    o.zi = zi;
    o.ar = ar;
    o.ai = ai;
    o.e = e;
    o.th = st.theta;
    if (p.open_loop) st.theta = 0.0;
}

// ------------------------------------------------------------------------------------------------------------------ the plan
struct Plan {
    int fam = 0, type = 0, c64 = 0, outs = kOutAll;
    int at_x = 0, at_a = 0, at_e = 0, at_t = 0, lds_doubles = 0;   // the LDS image in doubles: samples (and z' over them), a_hat, e_phi, theta_h
    int64_t n = 0, nrow = 0, start = 0, step = 1, x_stride = 0, y_stride = 0, tiles = 0, groups = 0;
};
inline const char *plan_make(int fam, int mod, int type, int dtype, int outs, int64_t n, int64_t nrow, int64_t start, int64_t step, int64_t x_stride, int64_t y_stride, Plan *p)
{
    if (const char *why = sym::order_check(fam, mod)) return why;
    if (type < 0 || type > 2) return "the detector type must be 0, 1 or 2";
    if (dtype != 1 && dtype != 3) return "complex64 or complex128 samples";
    if (outs < 1 || outs > kOutAll) return "at least one of z_prime, a_hat, e_phi, theta_h";
    if (n < 0 || nrow < 0 || n >= kMaxLen || nrow >= kMaxLen) return "need 0 <= n, nrow < 2^40";
    if (start < 0 || start >= kMaxLen || step < 1 || step >= ((int64_t)1 << 20)) return "need 0 <= start < 2^40 and 1 <= step < 2^20";
    if (x_stride < 0 || y_stride < n || x_stride >= kMaxLen || y_stride >= kMaxLen) return "need 0 <= x_stride and n <= y_stride, both below 2^40";
    if (n > 0 && x_stride < start + (n - 1) * step + 1) return "x_stride is smaller than the window a row is read from";
    p->fam = fam;
    p->type = type;
    p->c64 = dtype == 1;
    p->outs = outs;
    const int cplx = 2 * kLane * kPitch, real = kLane * kPitch;
    p->at_x = 0;
    p->at_a = cplx;
    p->at_e = p->at_a + ((outs & kOutA) ? cplx : 0);
    p->at_t = p->at_e + ((outs & kOutE) ? real : 0);
    p->lds_doubles = p->at_t + ((outs & kOutT) ? real : 0);
    p->n = n;
    p->nrow = nrow;
    p->start = start;
    p->step = step;
    p->x_stride = x_stride;
    p->y_stride = y_stride;
    p->tiles = (n + kTile - 1) / kTile;
    p->groups = (nrow + kLane - 1) / kLane;
    if (p->groups > (((int64_t)1 << 31) - 1)) return "too many rows for one launch";
    return nullptr;
}
// tab_re, tab_im: where the walk will read the decision points (MPSK above 4; not read otherwise)
inline void loop_make(int fam, int mod, int open_loop, double inv_sqrt2, const double *tab_re, const double *tab_im, Loop *p)
{
    p->mod = mod;
    p->x_m = fam == sym::kQam ? (mod == 2 ? 1 : (1 << (sym::bps_of(fam, mod) / 2)) - 1) : 0;
    p->open_loop = open_loop ? 1 : 0;
    p->inv_sqrt2 = inv_sqrt2;
    p->tab_re = tab_re;
    p->tab_im = tab_im;
}

struct Sample {     // an element as loaded: complex128 (re, im); complex64: its 8 bytes in `re`, widened by tile_put -- a conversion in tile_fetch would wait for the load
    double re, im;
};
// where element j of lane t lies in the tile: row e / kTile of the group, symbol e mod kTile of the tile, e = j 64 + t
SK_HD int elem_row(int t, int j) { return (j * kLane + t) / kTile; }
SK_HD int elem_sym(int t, int j) { return (j * kLane + t) % kTile; }
SK_HD int tile_count(const Plan &p, int64_t tile)
{
    const int64_t left = p.n - tile * kTile;
    return left < kTile ? (int)left : kTile;
}

// (C64 of the three movers below: the plan's c64, a compile-time constant -- a run-time branch per element makes the compiler wait for each load in turn)
// Lane t's share of a tile's loads, into registers.  Mem: ld_u64 (8 bytes as they lie) and ld_c128.  What lies outside the rows or the frame is not read.
template <bool C64, class Mem> SK_HD void tile_fetch(const Mem &m, const Plan &p, const void *x, int64_t group, int64_t tile, int t, Sample *regs)
{
    const int cnt = tile_count(p, tile);
    SK_UNROLL
    for (int j = 0; j < kPer; ++j) {
        const int64_t row = group * kLane + elem_row(t, j);
        const int k = elem_sym(t, j);
        regs[j].re = regs[j].im = 0.0;
        if (row < p.nrow && k < cnt) {
            const int64_t at = row * p.x_stride + p.start + (tile * kTile + k) * p.step;
            if (C64) regs[j].re = chan::bits_to_double(m.ld_u64(static_cast<const float *>(x) + 2 * at));
            else m.ld_c128(static_cast<const double *>(x) + 2 * at, &regs[j].re, &regs[j].im);
        }
    }
}
// the registers into the LDS image (every slot of the tile: the walk reads only what was loaded).  Lds: st2(i, a, b) writes doubles i, i + 1 (i even)
template <bool C64, class Lds> SK_HD void tile_put(const Plan &p, int t, const Sample *regs, const Lds &L)
{
    SK_UNROLL
    for (int j = 0; j < kPer; ++j) {
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
        L.st2(p.at_x + 2 * (elem_row(t, j) * kPitch + elem_sym(t, j)), re, im);
    }
}
// Lane t walks its row through the tile: the serial chain.  Lds: ld2 / st2 / st.
template <int FAM, int TYPE, class Lds> SK_HD void tile_walk(const Plan &p, const Loop &lp, const Row &w, int64_t group, int64_t tile, int t, State &st, const Lds &L)
{
    if (group * kLane + t >= p.nrow) return;
    const int cnt = tile_count(p, tile);
    const int base = t * kPitch;
    for (int k = 0; k < cnt; ++k) {
        double xr, xi;
        L.ld2(p.at_x + 2 * (base + k), &xr, &xi);
        StepOut o;
        step<FAM, TYPE>(lp, w, st, xr, xi, o);
        if (p.outs & kOutZ) {
            if (FAM == sym::kQam) {
                SK_NO_CONTRACT
                o.zr = o.zr * w.back;
                o.zi = o.zi * w.back;
            }
            L.st2(p.at_x + 2 * (base + k), o.zr, o.zi);
        }
        if (p.outs & kOutA) L.st2(p.at_a + 2 * (base + k), o.ar, o.ai);
        if (p.outs & kOutE) L.st(p.at_e + base + k, o.e);
        if (p.outs & kOutT) L.st(p.at_t + base + k, o.th);
    }
}
// Lane t's share of a tile's stores: the selected outputs as runs along the rows.  Mem: st_c64 / st_c128 / st_f64.  Lds: ld2 / ld.
template <bool C64, class Mem, class Lds> SK_HD void tile_store(const Mem &m, const Plan &p, void *z, void *a, double *e, double *th, int64_t group, int64_t tile, int t, const Lds &L)
{
    const int cnt = tile_count(p, tile);
    SK_UNROLL
    for (int j = 0; j < kPer; ++j) {
        const int rl = elem_row(t, j), k = elem_sym(t, j);
        const int64_t row = group * kLane + rl;
        if (row >= p.nrow || k >= cnt) continue;
        const int64_t at = row * p.y_stride + tile * kTile + k;
        const int slot = rl * kPitch + k;
        double re, im;
        if (p.outs & kOutZ) {
            L.ld2(p.at_x + 2 * slot, &re, &im);
            if (C64) m.st_c64(static_cast<float *>(z) + 2 * at, (float)re, (float)im);
            else m.st_c128(static_cast<double *>(z) + 2 * at, re, im);
        }
        if (p.outs & kOutA) {
            L.ld2(p.at_a + 2 * slot, &re, &im);
            if (C64) m.st_c64(static_cast<float *>(a) + 2 * at, (float)re, (float)im);
            else m.st_c128(static_cast<double *>(a) + 2 * at, re, im);
        }
        if (p.outs & kOutE) m.st_f64(e + at, L.ld(p.at_e + slot));
        if (p.outs & kOutT) m.st_f64(th + at, L.ld(p.at_t + slot));
    }
}
// a row's constants: gains: null (k1, k2 serve every row) or [nrow][2]; r: null (MPSK) or [nrow], the scale's reciprocal
template <class Mem> SK_HD Row row_of(const Mem &m, double k1, double k2, const double *gains, const double *r, int64_t row, int64_t nrow)
{
    Row w = {k1, k2, 1.0, 1.0};
    if (row >= nrow) return w;
    if (gains) {
        w.k1 = m.ld_f64(gains + 2 * row);
        w.k2 = m.ld_f64(gains + 2 * row + 1);
    }
    if (r) {
        w.r = m.ld_f64(r + row);
        w.back = 1.0 / w.r;
    }
    return w;
}

// ------------------------------------------------------------------------------------------------------------------ phase_step / time_step over rows
// mode 0, time_step:   y[r, j] = x[r, j] for j < a = min(n, ns n_step), else x[r, j + t_r] where that lies inside the row, else 0;  j < n_out
// mode 1, phase_step:  y[r, j] = x[r, j ns] f, f = 1 + 0j for j < n_step, the host's exp(1j p_r) from there on: re = a c - b d, im = a d + b c
struct ImpPlan {
    int mode = 0, c64 = 0;
    int64_t n = 0, n_out = 0, nrow = 0, ns = 1, n_step = 0, x_stride = 0, y_stride = 0;
};
inline const char *imp_plan_make(int mode, int dtype, int64_t n, int64_t n_out, int64_t nrow, int64_t ns, int64_t n_step, int64_t x_stride, int64_t y_stride, ImpPlan *p)
{
    if (mode != 0 && mode != 1) return "the mode must be 0 (time_step) or 1 (phase_step)";
    if (dtype != 1 && dtype != 3) return "complex64 or complex128 samples";
    if (n < 0 || nrow < 0 || n_out < 0 || n >= kMaxLen || nrow >= kMaxLen || n_out >= kMaxLen) return "need 0 <= n, n_out, nrow < 2^40";
    if (ns < 1 || ns >= ((int64_t)1 << 20) || n_step < 0 || n_step >= kMaxLen) return "need 1 <= ns < 2^20 and 0 <= n_step < 2^40";
    if (x_stride < n || y_stride < n_out || x_stride >= kMaxLen || y_stride >= kMaxLen) return "need n <= x_stride and n_out <= y_stride, both below 2^40";
    if (mode == 1 && n_out != (n + ns - 1) / ns) return "phase_step: n_out must be ceil(n / ns)";
    p->mode = mode;
    p->c64 = dtype == 1;
    p->n = n;
    p->n_out = n_out;
    p->nrow = nrow;
    p->ns = ns;
    p->n_step = n_step;
    p->x_stride = x_stride;
    p->y_stride = y_stride;
    return nullptr;
}
// output j of row `row`.  shift: the row's t_step (mode 0); (c, d): the row's factor (mode 1)
template <class Mem> SK_HD void imp_item(const Mem &m, const ImpPlan &p, const void *x, void *y, int64_t row, int64_t j, int64_t shift, double c, double d)
{
    SK_NO_CONTRACT
    double re = 0.0, im = 0.0;
    if (p.mode == 0) {
        const int64_t edge = p.ns * p.n_step < p.n ? p.ns * p.n_step : p.n;
        if (j < edge)
            sym::load_sym(m, x, row * p.x_stride + j, p.c64, &re, &im);
        else if (shift >= 0 && j < p.n && shift < p.n - j)      // (a shift no caller should pass reads nothing)
            sym::load_sym(m, x, row * p.x_stride + j + shift, p.c64, &re, &im);
    } else {
        double a, b;
        sym::load_sym(m, x, row * p.x_stride + j * p.ns, p.c64, &a, &b);
        if (j < p.n_step) {
            c = 1.0;
            d = 0.0;
        }
        re = a * c - b * d;
        im = a * d + b * c;
    }
    const int64_t at = row * p.y_stride + j;
    if (p.c64) m.st_c64(static_cast<float *>(y) + 2 * at, (float)re, (float)im);
    else m.st_c128(static_cast<double *>(y) + 2 * at, re, im);
}

}  // namespace car
}  // namespace skdsp
