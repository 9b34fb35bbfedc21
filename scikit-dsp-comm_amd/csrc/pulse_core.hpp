// pulse_core.hpp -- the plans and the per-thread functions of the two filtering stages of a single-carrier BER loop over a frame set: pulse shaping,
// lfilter(b, 1, upsample(s, ns)) (sigsys.py:2163-2211, digitalcom.py:1676, 1821 of the reference), and the matched filter read at the symbol rate,
// lfilter(b, 1, x)[start::step].  A row is a frame that starts from rest.  Plain C++ for host and device: pulse.hip builds its kernels from it and
// tests/host/pulse_emul.cpp walks the same functions thread by thread without a GPU.
//
// Semantics.   shaping:         y[r, k ns + p] = c * sum_j b[p + j ns] s[r, k - j],    0 <= p < ns, 0 <= k < n, every j with p + j ns < ntaps
//              matched filter:  z[r, k]        = sum_i b[i] x[r, start + k step - i],  0 <= k < n_out = max(0, ceil((n - start) / step))
// with s[r, < 0] = x[r, < 0] = 0.  b is real float64; signals are float32 / complex64 / float64 / complex128.
//
// Arithmetic: ONE recipe for every dtype, which sigsys.pulse_shape_rows_host / matched_filter_rows_host restate in NumPy and reproduce bit for bit.
// Elements are widened exactly at the load; products and sums are float64 and never contracted; the terms of an output are added from the oldest
// sample to the newest (largest j / i first) as acc = b x + acc, starting from +0, real and imaginary parts apart; terms that meet a sample in
// front of the row are computed (b * 0) like any other; the optional factor c multiplies each component once behind the sum; one rounding to the
// output dtype at the store.
//
// Geometry.  Both kernels: workgroups of 256 threads (four wave64), one (row, tile) each, the taps and the tile's samples staged in LDS as float64
// planes (re, im), plain vector loads and stores, no atomics.  The plan -- tile, grid, LDS words -- is a function of the sizes alone.
//   shaping         a tile is T = floor(2048 / ns) symbols and the H = ceil(ntaps / ns) - 1 symbols in front of it; thread t produces outputs
//                   t, t + 256, ... of the tile's T ns: consecutive lanes, consecutive samples, whole runs per store.  A lane's taps are phase
//                   o mod ns of b (consecutive lanes, consecutive words); the ns lanes of a symbol read one LDS address (a broadcast).
//   matched filter  a tile is To outputs and the W = (To - 1) step + ntaps samples they read.  Thread t holds R outputs t + 256 u in registers
//                   (R = 4, 2, 1 for step <= 4, <= 8, above; To = min(256 R, floor(4096 / step))) and walks the taps once for all of them: one
//                   broadcast tap read per R sample reads.  Neighbouring lanes read samples `step` apart -- a `step`-way bank conflict in the
//                   natural order for a power of two -- so the staging store swizzles: sample e of the window goes to plane e mod step, position
//                   e / step, re and im side by side.  The samples a wave reads for one tap are then 64 consecutive 16-byte (8-byte: real)
//                   words, one read per complex sample, and the position is a walk common to all lanes plus the lane's output index.
#pragma once
#include <math.h>
#include <stdint.h>
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#ifndef SK_HD
#define SK_HD __host__ __device__ __forceinline__
#endif
#else
#ifndef SK_HD
#define SK_HD inline
#endif
#endif
#ifndef SK_NO_CONTRACT
#if defined(__clang__)
#define SK_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define SK_NO_CONTRACT   // (a host compiler other than clang: build with -ffp-contract=off, as the tests do)
#endif
#endif
#if defined(__HIP_DEVICE_COMPILE__)
#define SK_UNROLL _Pragma("unroll")
#else
#define SK_UNROLL
#endif

namespace skdsp {
namespace pls {

constexpr int kThreads = 256, kLane = 64;
constexpr int kMaxTaps = 2049, kMaxRate = 64;          // the served range: ntaps, and ns / step
constexpr int kShapeOut = 2048;                        // output samples of a shaping tile, at most
constexpr int kMfIn = 4096, kMfMaxR = 4;               // input span of a matched-filter tile's outputs, at most; outputs a lane holds, at most
constexpr int64_t kMaxLen = (int64_t)1 << 40;

SK_HD int elem_bytes(int dtype) { return dtype == 0 ? 4 : dtype == 3 ? 16 : 8; }
SK_HD bool is_complex(int dtype) { return dtype == 1 || dtype == 3; }
inline bool served(int64_t rate, int64_t ntaps) { return rate >= 1 && rate <= kMaxRate && ntaps >= 1 && ntaps <= kMaxTaps; }
inline int64_t mf_out_len(int64_t n, int64_t start, int64_t step) { return n > start ? (n - start + step - 1) / step : 0; }

// one element, widened: dtype codes are the library's (0 float32, 1 complex64, 2 float64, 3 complex128).  Mem: ld_f32 / ld_f64 (one component),
// ld_c64 / ld_c128 (element i of an interleaved array) and the four stores below
template <class Mem> SK_HD void load_elem(const Mem &m, const void *p, int dtype, int64_t i, double *re, double *im)
{
    if (dtype == 0) {
        *re = m.ld_f32(static_cast<const float *>(p) + i);
        *im = 0.0;
    } else if (dtype == 1) {
        m.ld_c64(static_cast<const float *>(p) + 2 * i, re, im);
    } else if (dtype == 2) {
        *re = m.ld_f64(static_cast<const double *>(p) + i);
        *im = 0.0;
    } else {
        m.ld_c128(static_cast<const double *>(p) + 2 * i, re, im);
    }
}
// the one rounding to the output dtype
template <class Mem> SK_HD void store_elem(const Mem &m, void *p, int dtype, int64_t i, double re, double im)
{
    if (dtype == 0)
        m.st_f32(static_cast<float *>(p) + i, (float)re);
    else if (dtype == 1)
        m.st_c64(static_cast<float *>(p) + 2 * i, (float)re, (float)im);
    else if (dtype == 2)
        m.st_f64(static_cast<double *>(p) + i, re);
    else
        m.st_c128(static_cast<double *>(p) + 2 * i, re, im);
}

// acc = b x + acc: two roundings (FMA false, the recipe) or one (FMA true: the timing A/B only)
template <bool FMA> SK_HD double mac(double b, double x, double acc)
{
    SK_NO_CONTRACT
    if (FMA) return fma(b, x, acc);
    const double prod = b * x;
    return prod + acc;
}
SK_HD double scaled(double v, double c)
{
    SK_NO_CONTRACT
    return v * c;
}

// the rules both calls share; nullptr or what is wrong
inline const char *rows_check(int dtype, int64_t n, int64_t nrow, int64_t n_out, int64_t x_stride, int64_t y_stride)
{
    if (dtype < 0 || dtype > 3) return "float32, complex64, float64 or complex128 signals";
    if (n < 0 || nrow < 0 || n >= kMaxLen || nrow >= kMaxLen) return "need 0 <= n, nrow < 2^40";
    if (n_out >= kMaxLen) return "rows of fewer than 2^40 output samples";
    if (x_stride < n) return "x_stride is smaller than a row of the input";
    if (y_stride < n_out) return "y_stride is smaller than a row of the output";
    if (x_stride >= kMaxLen || y_stride >= kMaxLen) return "strides below 2^40";
    return nullptr;
}
inline bool grid_fits(int64_t tiles, int64_t nrow) { return tiles == 0 || nrow <= (((int64_t)1 << 31) - 1) / tiles; }

// ------------------------------------------------------------------------------------------------------------------ shaping
struct ShapePlan {
    int dtype = 0, cplx = 0, ns = 1, ntaps = 1, has_scale = 0;
    int J = 1, H = 0, T = 1;                     // taps of the longest phase, symbols in front of a tile, symbols of a tile
    int at_re = 0, at_im = 0, lds_doubles = 0;   // the LDS image in doubles: taps at 0, then the planes of T + H symbols
    int64_t n = 0, nrow = 0, x_stride = 0, y_stride = 0, tiles = 0;   // tiles per row
    double c = 1.0;
};
// ns and ntaps inside the served range (the caller has asked served())
inline const char *shape_plan_make(int dtype, int ntaps, int64_t ns, int64_t n, int64_t nrow, int64_t x_stride, int64_t y_stride, int has_scale, double c, ShapePlan *p)
{
    if (n < 0 || n >= kMaxLen) return "need 0 <= n, nrow < 2^40";
    if (const char *why = rows_check(dtype, n, nrow, n * ns, x_stride, y_stride)) return why;
    p->dtype = dtype;
    p->cplx = is_complex(dtype) ? 1 : 0;
    p->ns = (int)ns;
    p->ntaps = ntaps;
    p->has_scale = has_scale ? 1 : 0;
    p->c = has_scale ? c : 1.0;
    p->J = (ntaps + p->ns - 1) / p->ns;
    p->H = p->J - 1;
    p->T = kShapeOut / p->ns;
    p->at_re = ntaps;
    p->at_im = p->at_re + p->T + p->H;
    p->lds_doubles = p->at_im + (p->cplx ? p->T + p->H : 0);
    p->n = n;
    p->nrow = nrow;
    p->x_stride = x_stride;
    p->y_stride = y_stride;
    p->tiles = (n + p->T - 1) / p->T;
    if (!grid_fits(p->tiles, nrow)) return "too many (row, tile) pairs for one launch";
    return nullptr;
}

// Thread t's share of staging a tile: the taps, then symbols tile T - H ... tile T + T - 1 of the row (zeros outside [0, n)).  x_row: element 0 of the row.
// Lds: ld(i) / st(i, v) on the image of lds_doubles doubles.
template <class Mem, class Lds> SK_HD void shape_stage(const Mem &m, const ShapePlan &p, const double *taps, const void *x_row, int64_t tile, int t, const Lds &L)
{
    for (int i = t; i < p.ntaps; i += kThreads) L.st(i, m.ld_f64(taps + i));
    const int64_t k0 = tile * p.T - p.H;
    for (int i = t; i < p.T + p.H; i += kThreads) {
        const int64_t k = k0 + i;
        double re = 0.0, im = 0.0;
        if (k >= 0 && k < p.n) load_elem(m, x_row, p.dtype, k, &re, &im);
        L.st(p.at_re + i, re);
        if (p.cplx) L.st(p.at_im + i, im);
    }
}
// behind a barrier: thread t's outputs of the tile.  y_row: element 0 of the output row.
template <class Mem, class Lds> SK_HD void shape_outputs(const Mem &m, const ShapePlan &p, void *y_row, int64_t tile, int t, const Lds &L)
{
    const int64_t left = p.n - tile * p.T;
    const int valid = (int)(left < p.T ? left : p.T) * p.ns;
    const int64_t o0 = tile * p.T * p.ns;
    for (int o = t; o < valid; o += kThreads) {
        const int kl = o / p.ns, ph = o - kl * p.ns;
        double re = 0.0, im = 0.0;
        if (ph < p.ntaps) {
            for (int j = (p.ntaps - 1 - ph) / p.ns; j >= 0; --j) {    // oldest symbol first
                const double b = L.ld(ph + j * p.ns);
                re = mac<false>(b, L.ld(p.at_re + p.H + kl - j), re);
                if (p.cplx) im = mac<false>(b, L.ld(p.at_im + p.H + kl - j), im);
            }
        }
        if (p.has_scale) {
            re = scaled(re, p.c);
            im = scaled(im, p.c);
        }
        store_elem(m, y_row, p.dtype, o0 + o, re, im);
    }
}

// ------------------------------------------------------------------------------------------------------------------ matched filter
struct MfPlan {
    int dtype = 0, cplx = 0, comps = 1, ntaps = 1, step = 1, naive = 0;
    int R = 1, To = 1, W = 1, Wq = 1;            // outputs a lane holds, outputs of a tile, samples a tile stages, positions of a phase plane
    int at_x = 0, lds_doubles = 0;               // taps at 0, then the window from an even word on: `comps` doubles (re, im) per position
    int64_t n = 0, n_out = 0, nrow = 0, start = 0, x_stride = 0, y_stride = 0, tiles = 0;
};
// where window sample e lives: in the plane of its phase e mod step, at e / step -- the samples neighbouring lanes read, `step` apart, are neighbours
// in the image.  Planes are Wq positions apart, Wq odd: the staging stores of consecutive samples spread over the banks too.  naive: at e.
SK_HD int mf_pos(const MfPlan &p, int e) { return p.naive ? e : (e % p.step) * p.Wq + e / p.step; }
// step and ntaps inside the served range; naive: the window in its natural order (timing A/B)
inline const char *mf_plan_make(int dtype, int ntaps, int64_t n, int64_t nrow, int64_t start, int64_t step, int64_t x_stride, int64_t y_stride, int naive, MfPlan *p)
{
    if (start < 0 || start >= kMaxLen) return "need 0 <= start < 2^40";
    if (n < 0 || n >= kMaxLen) return "need 0 <= n, nrow < 2^40";
    const int64_t n_out = mf_out_len(n, start, step);
    if (const char *why = rows_check(dtype, n, nrow, n_out, x_stride, y_stride)) return why;
    p->dtype = dtype;
    p->cplx = is_complex(dtype) ? 1 : 0;
    p->comps = p->cplx ? 2 : 1;
    p->ntaps = ntaps;
    p->step = (int)step;
    p->naive = naive ? 1 : 0;
    p->R = step <= 4 ? 4 : step <= 8 ? 2 : 1;
    const int span = kMfIn / p->step;
    p->To = kThreads * p->R < span ? kThreads * p->R : span;
    p->W = (p->To - 1) * p->step + ntaps;
    p->Wq = ((p->W + p->step - 1) / p->step) | 1;
    p->at_x = (ntaps + 1) & ~1;
    p->lds_doubles = p->at_x + p->comps * (p->naive ? p->W : p->step * p->Wq);
    p->n = n;
    p->n_out = n_out;
    p->nrow = nrow;
    p->start = start;
    p->x_stride = x_stride;
    p->y_stride = y_stride;
    p->tiles = (n_out + p->To - 1) / p->To;
    if (!grid_fits(p->tiles, nrow)) return "too many (row, tile) pairs for one launch";
    return nullptr;
}

// Thread t's share of staging a tile: the taps, then x[g0 ... g0 + W) of the row with g0 = start + tile To step - (ntaps - 1) (zeros outside [0, n))
template <class Mem, class Lds> SK_HD void mf_stage(const Mem &m, const MfPlan &p, const double *taps, const void *x_row, int64_t tile, int t, const Lds &L)
{
    for (int i = t; i < p.ntaps; i += kThreads) L.st(i, m.ld_f64(taps + i));
    const int64_t g0 = p.start + tile * p.To * p.step - (p.ntaps - 1);
    for (int i = t; i < p.W; i += kThreads) {
        const int64_t g = g0 + i;
        double re = 0.0, im = 0.0;
        if (g >= 0 && g < p.n) load_elem(m, x_row, p.dtype, g, &re, &im);
        const int at = p.at_x + p.comps * mf_pos(p, i);
        L.st(at, re);
        if (p.cplx) L.st(at + 1, im);
    }
}
// behind a barrier: thread t's outputs t + 256 u (u < R) of the tile; a lane beyond the tile's last output repeats that output and stores nothing.
// Output q reads window samples q step + c, c = 0 (the oldest, tap ntaps - 1) ... ntaps - 1: position (c mod step) Wq + c / step + q -- a walk that is
// the same for every lane, plus the lane's q.  Lds: ld2(i, &a, &b) reads doubles i, i + 1 (i even).
template <int R, bool FMA, bool CPLX, class Mem, class Lds> SK_HD void mf_outputs(const Mem &m, const MfPlan &p, void *y_row, int64_t tile, int t, const Lds &L)
{
    const int64_t left = p.n_out - tile * p.To;
    const int valid = (int)(left < p.To ? left : p.To);
    if (t >= valid) return;
    int mine[R];                                 // the lane's part of a position
    double re[R], im[R];
    SK_UNROLL
    for (int u = 0; u < R; ++u) {
        const int q = t + kThreads * u < valid ? t + kThreads * u : valid - 1;
        mine[u] = p.naive ? q * p.step : q;
        re[u] = im[u] = 0.0;
    }
    int walk = 0, r = 0;                         // (c mod step) Wq + c / step
    for (int c = 0; c < p.ntaps; ++c) {          // oldest sample first
        const double b = L.ld(p.ntaps - 1 - c);
        const int base = p.naive ? c : walk;
        SK_UNROLL
        for (int u = 0; u < R; ++u) {
            if (CPLX) {
                double xr, xi;
                L.ld2(p.at_x + 2 * (base + mine[u]), &xr, &xi);
                re[u] = mac<FMA>(b, xr, re[u]);
                im[u] = mac<FMA>(b, xi, im[u]);
            } else {
                re[u] = mac<FMA>(b, L.ld(p.at_x + base + mine[u]), re[u]);
            }
        }
        if (++r == p.step) {
            r = 0;
            walk -= (p.step - 1) * p.Wq - 1;
        } else {
            walk += p.Wq;
        }
    }
    SK_UNROLL
    for (int u = 0; u < R; ++u) {
        const int q = t + kThreads * u;
        if (q < valid) store_elem(m, y_row, p.dtype, tile * p.To + q, re[u], im[u]);
    }
}

}  // namespace pls
}  // namespace skdsp
