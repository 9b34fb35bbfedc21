// symerr_core.hpp -- the plans, the index algebra, the quantiser and the per-element decision functions of the symbol-error kernels behind
// digitalcom.xcorr (digitalcom.py:1163-1179 of the reference), qam_sep (:495-582), qpsk_bep (:723-790) and bpsk_bep (:793-846).  Plain C++ for
// host and device: symerr.hip builds its kernels from it and tests/host/symerr_emul.cpp walks the same functions thread by thread without a GPU.
//
// The lag-window correlation.  R[l] = sum_{n < K} a[(n + l) mod K] conj(b[n]), K = 2 floor(len / 2), for the lags the reference keeps behind its
// fftshift: l = l0 ... l0 + nl - 1 with l0 = -min(n_lags, K / 2) and nl = min(2 n_lags + 1, K), plus E1 = sum |a|^2 and E2 = sum |b|^2.  Elements are
// widened at the load and every sum is float64, so integer-valued streams give exact integers in any order of summation.  With `quant` = M levels
// an element of a passes through qam_sep's quantiser first: 2 clip(rint((M - 1)(v + 1) / 2), 0, M - 1) - (M - 1) on each component.
//
// Geometry.  A workgroup of 4 waves owns a GROUP of kLagsWg = 256 consecutive lags and a PARTITION of the sample tiles.  Per tile of kTile = 1024
// samples it stages b[n0 .. n0 + 1024) and the window a[(n0 + first lag of the group + i) mod K], i < 1280, in LDS as re / im planes.  Wave w
// takes samples 256 w ... 256 w + 255 of the tile; lane ln holds the sums of lags ln + 64 j (j < 4) in registers and, per step n < 64, multiplies
// them with samples n + 64 s (s < 4): the 16 products need 7 window values a[n + ln + 64 (j + s)] (consecutive lanes, consecutive words: no bank
// conflict) and 4 values of b (one address per wave: a broadcast) -- 22 LDS reads for 64 FMAs.  The waves' sums are added in wave order, one
// partial per (partition, lag) goes to scratch, and a second kernel adds the partitions in their order: no float atomics, two runs are identical.
// The number of partitions is a function of (K, nl) alone (lag_plan_make): scratch is at most kMaxParts partials per lag.
//
// The count.  A work item is (row, 2048 symbols); thread t takes symbols t, t + 256, ...: adjacent lanes, adjacent symbols.  tx symbol i is
// tx[t0 + i], rx symbol i is x[start + (r0 + i) step] of its row, rotated by (1j)^k (BPSK: (-1)^k) -- swaps and negations.  Sums are integers:
// lanes, waves and the workgroup are reduced first, then four integer atomics per work item.
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
namespace sye {

constexpr int kThreads = 256, kLane = 64, kWaves = kThreads / kLane;
constexpr int kRL = 4, kRS = 4;                       // lags x samples a lane multiplies per step
constexpr int kLagsWg = kLane * kRL;                  // lags per group: 256
constexpr int kTile = kWaves * kLane * kRS;           // samples per tile: 1024
constexpr int kWin = kTile + kLagsWg;                 // window of a per tile: 1280 (1279 are read)
constexpr int kTargetWgs = 1024, kMaxParts = 128;     // the plan aims at this many workgroups with at most this many partitions
// LDS image in doubles: the planes of the window and of the tile; the waves' sums and the energies reuse the window's planes
constexpr int kSaRe = 0, kSaIm = kWin, kSbRe = 2 * kWin, kSbIm = 2 * kWin + kTile, kLdsDoubles = 2 * kWin + 2 * kTile;
constexpr int kRed = 0, kRedE = 2 * kWaves * kLagsWg; // [wave][lag][re, im] then [2][thread]
static_assert(kRedE + 2 * kThreads <= kSaRe + 2 * kWin, "the reductions fit the window's planes");

enum Mode { kModeQam = 0, kModeQpsk = 1, kModeBpsk = 2 };
constexpr int kSymRun = 8, kSymWg = kThreads * kSymRun;   // symbols per lane and per work item of the count

SK_HD bool finite_d(double v) { return fabs(v) <= 1.7976931348623157e308; }
SK_HD int elem_bytes(int dtype) { return dtype == 0 ? 4 : dtype == 3 ? 16 : 8; }
inline bool levels_ok(int M) { return M == 2 || M == 4 || M == 8 || M == 16; }

// one element, widened: dtype codes are the library's (0 float32, 1 complex64, 2 float64, 3 complex128).  Mem: ld_f32 / ld_f64 (one component)
// and ld_c64 / ld_c128 (element i of an interleaved array)
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

// qam_sep's quantiser on one component (digitalcom.py:525-536): the reference's operations in its order; what is not a number stays so
SK_HD double quant(double v, int M)
{
    SK_NO_CONTRACT
    const double top = (double)(M - 1);
    double q = rint(top * (v + 1.0) / 2.0);
    if (q > top) q = top;
    if (q < 0.0) q = 0.0;
    return 2.0 * q - top;
}
// (re + j im) (1j)^k of finite values
SK_HD void rotate(int k, double *re, double *im)
{
    const double r = *re, i = *im;
    if (k == 1) {
        *re = -i;
        *im = r;
    } else if (k == 2) {
        *re = -r;
        *im = -i;
    } else if (k == 3) {
        *re = i;
        *im = -r;
    }
}

// ------------------------------------------------------------------------------------------------------------------ lag correlation
struct LagPlan {
    int64_t K = 0, nl = 0, l0 = 0;        // samples, lags, first lag
    int64_t ntiles = 0, tpp = 0;          // tiles, tiles per partition
    int ngroups = 0, nparts = 0;
    int a_dtype = 0, b_dtype = 0, quant = 0;
};
inline const char *lag_plan_make(int64_t len, int64_t n_lags, int a_dtype, int b_dtype, int quant_levels, LagPlan *p)
{
    if (a_dtype < 0 || a_dtype > 3 || b_dtype < 0 || b_dtype > 3) return "float32, complex64, float64 or complex128 streams";
    if (quant_levels != 0 && !levels_ok(quant_levels)) return "the quantiser takes 2, 4, 8 or 16 levels (0: none)";
    if (len < 0 || n_lags < 0 || len >= ((int64_t)1 << 40)) return "need 0 <= len < 2^40 and n_lags >= 0";
    const int64_t K = 2 * (len / 2), half = K / 2, nh = n_lags < half ? n_lags : half;
    const int64_t nl = n_lags >= half ? K : 2 * n_lags + 1;
    if (nl > ((int64_t)1 << 30)) return "at most 2^30 lags";
    p->K = K;
    p->nl = nl;
    p->l0 = -nh;
    p->ntiles = (K + kTile - 1) / kTile;
    p->ngroups = (int)((nl + kLagsWg - 1) / kLagsWg);
    int64_t want = p->ngroups ? (kTargetWgs + p->ngroups - 1) / p->ngroups : 1;
    if (want > kMaxParts) want = kMaxParts;
    if (want > p->ntiles) want = p->ntiles;
    if (want < 1) want = 1;
    p->tpp = p->ntiles ? (p->ntiles + want - 1) / want : 0;
    p->nparts = p->tpp ? (int)((p->ntiles + p->tpp - 1) / p->tpp) : 0;
    p->a_dtype = a_dtype;
    p->b_dtype = b_dtype;
    p->quant = quant_levels;
    return nullptr;
}
SK_HD int64_t lag_padded(const LagPlan &p) { return (int64_t)p.ngroups * kLagsWg; }
// scratch in doubles: [part][padded lag][re, im], then [part][E1, E2]
SK_HD int64_t lag_part_at(const LagPlan &p, int part, int64_t lag_index) { return 2 * ((int64_t)part * lag_padded(p) + lag_index); }
SK_HD int64_t lag_energy_at(const LagPlan &p, int part) { return 2 * (int64_t)p.nparts * lag_padded(p) + 2 * part; }
inline int64_t lag_scratch_doubles(const LagPlan &p) { return 2 * (int64_t)p.nparts * lag_padded(p) + 2 * p.nparts; }
SK_HD int64_t lag_tile_first(const LagPlan &p, int part) { return (int64_t)part * p.tpp; }
SK_HD int64_t lag_tile_end(const LagPlan &p, int part)
{
    const int64_t e = (int64_t)(part + 1) * p.tpp;
    return e < p.ntiles ? e : p.ntiles;
}
SK_HD int64_t lag_tile_valid(const LagPlan &p, int64_t tile)
{
    const int64_t left = p.K - tile * kTile;
    return left < kTile ? left : kTile;
}
// the element of a behind window entry 0 of (tile, group): (n0 + l0 + 256 g) mod K
SK_HD int64_t lag_window_base(const LagPlan &p, int64_t tile, int g)
{
    int64_t v = (tile * kTile + p.l0 + (int64_t)g * kLagsWg) % p.K;
    return v < 0 ? v + p.K : v;
}

struct LagAcc {
    double re[kRL], im[kRL];
};

// Thread t's share of staging (tile, group g).  Lds: ld(i) / st(i, v) on the image of kLdsDoubles doubles.
template <class Mem, class Lds> SK_HD void lag_stage(const Mem &m, const LagPlan &p, const void *a, const void *b, int64_t tile, int g, int t, const Lds &L)
{
    const int64_t n0 = tile * kTile, nv = lag_tile_valid(p, tile);
    for (int i = t; i < kTile; i += kThreads) {
        double re = 0.0, im = 0.0;
        if (i < nv) load_elem(m, b, p.b_dtype, n0 + i, &re, &im);
        L.st(kSbRe + i, re);
        L.st(kSbIm + i, im);
    }
    const int64_t base = lag_window_base(p, tile, g);
    for (int i = t; i < kWin; i += kThreads) {
        double re = 0.0, im = 0.0;
        if (i < nv + kLagsWg) {                    // (entries behind the last sample's last lag meet zeros of b only)
            int64_t idx = base + i;
            if (idx >= p.K) idx = p.K >= kWin ? idx - p.K : idx % p.K;
            load_elem(m, a, p.a_dtype, idx, &re, &im);
            if (p.quant) {
                re = quant(re, p.quant);
                im = quant(im, p.quant);
            }
        }
        L.st(kSaRe + i, re);
        L.st(kSaIm + i, im);
    }
}
// group 0 only: its window's entries i < nv are a[(n0 + l0 + i) mod K], every element of a exactly once over the tiles
template <class Lds> SK_HD void lag_energy(const LagPlan &p, int64_t tile, int t, const Lds &L, double *e1, double *e2)
{
    const int64_t nv = lag_tile_valid(p, tile);
    for (int i = t; i < nv; i += kThreads) {
        const double ar = L.ld(kSaRe + i), ai = L.ld(kSaIm + i), br = L.ld(kSbRe + i), bi = L.ld(kSbIm + i);
        *e1 = *e1 + (ar * ar + ai * ai);
        *e2 = *e2 + (br * br + bi * bi);
    }
}
// one staged tile into thread t's sums
template <class Lds> SK_HD void lag_mac(const LagPlan &p, int g, int t, const Lds &L, LagAcc &acc)
{
    const int w = t / kLane, ln = t % kLane;
    if ((int64_t)g * kLagsWg + ln >= p.nl) return;     // none of this lane's lags ln + 64 j is served
    const int at = w * (kLane * kRS);
    for (int n = 0; n < kLane; ++n) {
        double ar[kRL + kRS - 1], ai[kRL + kRS - 1], br[kRS], bi[kRS];
        SK_UNROLL
        for (int q = 0; q < kRL + kRS - 1; ++q) {
            ar[q] = L.ld(kSaRe + at + n + ln + kLane * q);
            ai[q] = L.ld(kSaIm + at + n + ln + kLane * q);
        }
        SK_UNROLL
        for (int s = 0; s < kRS; ++s) {
            br[s] = L.ld(kSbRe + at + n + kLane * s);
            bi[s] = L.ld(kSbIm + at + n + kLane * s);
        }
        SK_UNROLL
        for (int j = 0; j < kRL; ++j) {
            SK_UNROLL
            for (int s = 0; s < kRS; ++s) {            // a conj(b)
                acc.re[j] = acc.re[j] + ar[j + s] * br[s];
                acc.re[j] = acc.re[j] + ai[j + s] * bi[s];
                acc.im[j] = acc.im[j] + ai[j + s] * br[s];
                acc.im[j] = acc.im[j] - ar[j + s] * bi[s];
            }
        }
    }
}
// behind the last tile (and a barrier): thread t's sums and energies into the image
template <class Lds> SK_HD void lag_put(int t, const Lds &L, const LagAcc &acc, double e1, double e2)
{
    const int w = t / kLane, ln = t % kLane;
    SK_UNROLL
    for (int j = 0; j < kRL; ++j) {
        L.st(kRed + 2 * (w * kLagsWg + ln + kLane * j), acc.re[j]);
        L.st(kRed + 2 * (w * kLagsWg + ln + kLane * j) + 1, acc.im[j]);
    }
    L.st(kRedE + t, e1);
    L.st(kRedE + kThreads + t, e2);
}
// behind a barrier: thread t is lag t of the group; thread 0 of group 0 adds the energies in thread order.  Mem: st_f64x2 (16 bytes at a multiple of 16)
template <class Mem, class Lds> SK_HD void lag_store(const Mem &m, const LagPlan &p, int g, int part, int t, const Lds &L, double *scratch)
{
    const int64_t li = (int64_t)g * kLagsWg + t;
    if (li < p.nl) {
        double re = 0.0, im = 0.0;
        for (int w = 0; w < kWaves; ++w) {
            re = re + L.ld(kRed + 2 * (w * kLagsWg + t));
            im = im + L.ld(kRed + 2 * (w * kLagsWg + t) + 1);
        }
        m.st_f64x2(scratch + lag_part_at(p, part, li), re, im);
    }
    if (g == 0 && t == 0) {
        double e1 = 0.0, e2 = 0.0;
        for (int u = 0; u < kThreads; ++u) {
            e1 = e1 + L.ld(kRedE + u);
            e2 = e2 + L.ld(kRedE + kThreads + u);
        }
        m.st_f64x2(scratch + lag_energy_at(p, part), e1, e2);
    }
}
// the second kernel: item i < nl is a lag, item nl the energies; partitions in their order.  Mem: ld_f64x2
template <class Mem> SK_HD void lag_merge_item(const Mem &m, const LagPlan &p, const double *scratch, int64_t i, double *r, double *e)
{
    if (i > p.nl) return;
    double re = 0.0, im = 0.0;
    for (int part = 0; part < p.nparts; ++part) {
        double x, y;
        m.ld_f64x2(scratch + (i < p.nl ? lag_part_at(p, part, i) : lag_energy_at(p, part)), &x, &y);
        re = re + x;
        im = im + y;
    }
    m.st_f64x2(i < p.nl ? r + 2 * i : e, re, im);
}

// ------------------------------------------------------------------------------------------------------------------ the count
struct CntPlan {
    int tx_dtype = 0, x_dtype = 0, mode = 0, M = 0, k = 0;
    int64_t tx_stride = 0, t0 = 0, x_stride = 0, start = 0, step = 1, r0 = 0, n = 0;
};
inline int64_t cnt_items_per_row(int64_t n) { return (n + kSymWg - 1) / kSymWg; }
inline const char *cnt_plan_make(int tx_dtype, int64_t tx_stride, int64_t t0, int x_dtype, int64_t x_stride, int64_t start, int64_t step, int64_t r0, int64_t n, int mode,
                                 int levels, int kphase, CntPlan *p)
{
    if (tx_dtype < 0 || tx_dtype > 3 || x_dtype < 0 || x_dtype > 3) return "float32, complex64, float64 or complex128 streams";
    if (mode != kModeQam && mode != kModeQpsk && mode != kModeBpsk) return "mode 0 (QAM), 1 (QPSK) or 2 (BPSK)";
    if (mode == kModeQam && !levels_ok(levels)) return "QAM of 2, 4, 8 or 16 levels per component";
    if (kphase < 0 || kphase > (mode == kModeBpsk ? 1 : 3)) return "the rotation is 0 ... 3 (BPSK: 0 or 1)";
    if (n < 0 || tx_stride < 0 || x_stride < 0 || t0 < 0 || start < 0 || r0 < 0 || step < 1) return "need n, strides, offsets >= 0 and step >= 1";
    if (n >= ((int64_t)1 << 40) || step >= ((int64_t)1 << 20) || t0 >= ((int64_t)1 << 40) || r0 >= ((int64_t)1 << 40) || start >= ((int64_t)1 << 40))
        return "need n, offsets < 2^40 and step < 2^20";
    p->tx_dtype = tx_dtype;
    p->x_dtype = x_dtype;
    p->mode = mode;
    p->M = mode == kModeQam ? levels : 0;
    p->k = kphase;
    p->tx_stride = tx_stride;
    p->t0 = t0;
    p->x_stride = x_stride;
    p->start = start;
    p->step = step;
    p->r0 = r0;
    p->n = n;
    return nullptr;
}
// elements of a row that a call reads: [t0, t0 + n) of tx, start + (r0 + i) step of x
SK_HD int64_t cnt_tx_at(const CntPlan &p, int64_t i) { return p.t0 + i; }
SK_HD int64_t cnt_x_at(const CntPlan &p, int64_t i) { return p.start + (p.r0 + i) * p.step; }

struct Cnt {
    int32_t c[4];   // the sums of a lane's kSymRun symbols: |value| < 2^19
};
// int16((v + 1) / 2) of the reference; false where the cast is not defined
SK_HD bool half_level(double v, int *out)
{
    SK_NO_CONTRACT
    const double h = (v + 1.0) / 2.0;
    if (!(fabs(h) < 32768.0)) return false;
    *out = (int)h;
    return true;
}
SK_HD void sym_item(const CntPlan &p, double tr, double ti, double xr, double xi, Cnt &c)
{
    if (p.mode == kModeQam) {
        if (!(finite_d(tr) && finite_d(ti) && finite_d(xr) && finite_d(xi) && tr == rint(tr) && ti == rint(ti))) {
            c.c[3] += 1;
            return;
        }
        double qr = quant(xr, p.M), qi = quant(xi, p.M);
        rotate(p.k, &qr, &qi);
        c.c[0] += (qr != tr || qi != ti) ? 1 : 0;
    } else if (p.mode == kModeQpsk) {
        int tI, tQ, rI, rQ;
        if (!(finite_d(xr) && finite_d(xi))) {
            c.c[3] += 1;
            return;
        }
        rotate(p.k, &xr, &xi);
        if (!(half_level(tr, &tI) && half_level(ti, &tQ) && half_level(xr, &rI) && half_level(xi, &rQ))) {
            c.c[3] += 1;
            return;
        }
        const int eI = tI ^ rI, eQ = tQ ^ rQ;
        c.c[0] += eI;
        c.c[1] += eQ;
        c.c[2] += eI | eQ;
    } else {
        int tI, rI;
        if (!finite_d(xr)) {
            c.c[3] += 1;
            return;
        }
        if (p.k & 1) xr = -xr;
        if (!(half_level(tr, &tI) && half_level(xr, &rI))) {
            c.c[3] += 1;
            return;
        }
        c.c[0] += tI ^ rI;
    }
}
// thread t's symbols of work item `it` of a row; tx / x: element 0 of the row
template <class Mem> SK_HD void cnt_thread(const Mem &m, const CntPlan &p, const void *tx, const void *x, int64_t it, int t, Cnt &c)
{
    SK_UNROLL
    for (int u = 0; u < kSymRun; ++u) {
        const int64_t i = it * kSymWg + (int64_t)u * kThreads + t;
        if (i >= p.n) continue;
        double tr, ti, xr, xi;
        load_elem(m, tx, p.tx_dtype, cnt_tx_at(p, i), &tr, &ti);
        load_elem(m, x, p.x_dtype, cnt_x_at(p, i), &xr, &xi);
        sym_item(p, tr, ti, xr, xi, c);
    }
}

}  // namespace sye
}  // namespace skdsp
