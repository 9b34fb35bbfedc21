// ofdm_core.hpp -- OFDM modulation and demodulation over the rows of a frame set: digitalcom.mux_pilot_blocks / ofdm_tx / chan_est_equalize /
// ofdm_rx (digitalcom.py:1284-1547 of the reference).  The argument rules, the carrier map, the pilot multiplex as index arithmetic and the
// per-thread phases of the kernels of ofdm.hip.  Same code for the device (hipcc, gfx950) and the host (g++: tests/host/ofdm_emul.cpp, where
// Mem checks every global access against the row's window and its alignment).
//
// The transform is psd_core.hpp's in-place float64 FFT with its geometry (256 threads, NB = 1024 / nc symbols side by side while nc <= 512,
// R = nc / 1024 butterflies per thread beyond): first() with a loader, mid(), and last_store() below, which is psd's last pass with its four
// points written back.  The spectrum stays in digit-reversed positions in LDS; pos_of() undoes the permutation on the LDS read that feeds the
// global store.  The inverse transform of the transmitter is the forward one between two conjugations, times the exact 1 / nc.
//
//   carrier c (0 <= c < nf)   ->  bin c + 1 for c < nf / 2, else bin nc - nf + c; bin 0 and every other bin are zero
//   muxed symbol j (npb > 0)  ->  a pilot (all ones) if j % npb == 0, else data symbol j - j / npb - 1; T = N + N / (npb - 1) + 1 symbols, and
//                                 where npb - 1 divides N the last one is all zeros, not a pilot (the reference assigns into an empty slice)
//   received symbol k         ->  samples x[k stride + off + n], (stride, off) = (nc + ncp, ncp) with a cyclic prefix, else (nc, 0)
//   npb > 0 at the receiver   ->  symbol k is a pilot if k % npb == 0 (row k / npb of the pilot buffer), else data row k - k / npb - 1
#pragma once
#include <math.h>
#include "psd_core.hpp"

namespace skdsp {
namespace ofdm {

using psd::cx;
using psd::kThreads;

template <int LOG2N> struct Core : psd::Core<double, double, LOG2N> {
    typedef psd::Core<double, double, LOG2N> P;
    static constexpr int N = P::N;

    // position of bin f: the inverse of bin_of
    static SK_HD int pos_of(int f)
    {
        int p = 0, q = N;
        SK_UNROLL
        for (int s = 0; s < P::NP4; ++s) {
            q >>= 2;
            p += (f & 3) * q;
            f >>= 2;
        }
        if (P::ODD) p += f & 1;
        return p;
    }

    // the last pass (radix 4, or radix 2 for an odd log2 N), its four points written back
    static SK_HD void last_store(int t, cx<double> *img)
    {
        SK_UNROLL
        for (int i = 0; i < P::R; ++i) {
            const int base = 4 * (t + P::TS * i);
            cx<double> v[4];
            SK_UNROLL
            for (int m = 0; m < 4; ++m) v[m] = img[base + m];
            if (P::ODD) {
                const cx<double> a = v[0], b = v[1], c = v[2], d = v[3];
                v[0] = psd::cadd(a, b);
                v[1] = psd::csub(a, b);
                v[2] = psd::cadd(c, d);
                v[3] = psd::csub(c, d);
            } else {
                psd::dft4(v);
            }
            SK_UNROLL
            for (int m = 0; m < 4; ++m) img[base + m] = v[m];
        }
    }
};

SK_HD int carrier_of_bin(int n, int nf, int nc)   // -1: an unfilled bin
{
    const int h = nf >> 1;
    if (n >= 1 && n <= h) return n - 1;
    if (n >= nc - h) return n - (nc - nf);
    return -1;
}
SK_HD int bin_of_carrier(int c, int nf, int nc) { return c < (nf >> 1) ? c + 1 : nc - nf + c; }

// a / b as NumPy divides (Smith)
SK_HD cx<double> cdiv(cx<double> a, cx<double> b)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    if (fabs(b.x) >= fabs(b.y)) {
        const double r = b.y / b.x, den = b.x + b.y * r;
        return cx<double>{(a.x + a.y * r) / den, (a.y - a.x * r) / den};
    }
    const double r = b.x / b.y, den = b.x * r + b.y;
    return cx<double>{(a.x * r + a.y) / den, (a.y * r - a.x) / den};
}

// ---------------------------------------------------------------------------------------------------------------- the argument rules
inline int log2_of(int nc)
{
    int l = 0;
    while ((1 << l) < nc) ++l;
    return l;
}
// null, or why the shape is refused.  rx: npb = -1 (the known channel) is allowed and needs a table
inline const char *shape_why(int nf, int nc, int npb, int ncp, int rx, int has_table)
{
    if (nc < (1 << psd::kMinLog2) || nc > (1 << psd::kMaxLog2) || (nc & (nc - 1))) return "nc must be a power of two in 64 ... 4096";
    if (nf < 2 || (nf & 1) || nf > nc - 2) return "nf must be even, 2 ... nc - 2";
    if (npb == 1) return "npb = 1 leaves no data symbols";
    if (npb < (rx ? -1 : 0)) return rx ? "npb must be -1, 0 or at least 2" : "npb must be 0 or at least 2";
    if (ncp < 0 || ncp > nc) return "ncp must be 0 ... nc";
    if (rx && npb == -1 && !has_table) return "npb = -1 needs the channel";
    return nullptr;
}
inline int64_t tx_symbols(int64_t nsym, int npb) { return npb > 0 ? nsym + nsym / (npb - 1) + 1 : nsym; }
inline int64_t rx_pilots(int64_t nsym, int npb) { return npb > 0 ? (nsym + npb - 1) / npb : 0; }

struct TxPlan {
    int64_t nsym, T;            // data symbols in, symbols out (per row)
    int64_t x_stride, y_stride; // elements from row to row
    int64_t groups;             // per row: ceil(T / NB)
    int nf, nc, npb, ncp;       // ncp: 0 without a cyclic prefix
    int zero_last;              // the last muxed symbol is the zero row
};
inline void tx_plan_make(int64_t nsym, int nf, int nc, int npb, int cp, int ncp, int64_t x_stride, int64_t y_stride, TxPlan *p)
{
    const int nb = nc >= 1024 ? 1 : 1024 / nc;
    p->nsym = nsym;
    p->T = tx_symbols(nsym, npb);
    p->x_stride = x_stride;
    p->y_stride = y_stride;
    p->groups = (p->T + nb - 1) / nb;
    p->nf = nf;
    p->nc = nc;
    p->npb = npb;
    p->ncp = cp ? ncp : 0;
    p->zero_last = npb > 0 && nsym % (npb - 1) == 0;
}

struct RxPlan {
    int64_t nsym, npilot, ndata;   // symbols in, pilot and data symbols among them (per row)
    int64_t x_stride, z_stride;    // elements from row to row (z: of the output this launch writes)
    int64_t groups;
    int64_t stride;                // samples from symbol to symbol
    int nf, nc, npb, off;
};
inline void rx_plan_make(int64_t nsym, int nf, int nc, int npb, int cp, int ncp, int64_t x_stride, int64_t z_stride, RxPlan *p)
{
    const int nb = nc >= 1024 ? 1 : 1024 / nc;
    p->nsym = nsym;
    p->npilot = rx_pilots(nsym, npb);
    p->ndata = nsym - p->npilot;
    p->x_stride = x_stride;
    p->z_stride = z_stride;
    p->groups = (nsym + nb - 1) / nb;
    p->stride = cp ? nc + ncp : nc;
    p->nf = nf;
    p->nc = nc;
    p->npb = npb;
    p->off = cp ? ncp : 0;
}

// ---------------------------------------------------------------------------------------------------------------- the transmitter
// what muxed symbol j is: 0 data symbol *d, 1 a pilot, 2 zeros
SK_HD int mux_row(const TxPlan &p, int64_t j, int64_t *d)
{
    *d = j;
    if (p.npb <= 0) return 0;
    const int64_t q = j / p.npb;
    if (j == q * p.npb) return (p.zero_last && j == p.T - 1) ? 2 : 1;
    *d = j - q - 1;
    return 0;
}

// pass 0 of the group of symbols j0 .. j0 + NB - 1 of a row: the loader is the carrier map, read conjugated
template <typename SI, int LOG2N, class Mem>
SK_HD void tx_first(const Mem &mem, const TxPlan &p, const SI *xrow, int64_t j0, int tid, const cx<double> *tw, cx<double> *work)
{
    typedef Core<LOG2N> C;
    const int sb = tid / C::TS, t = tid % C::TS;
    const int64_t j = j0 + sb;
    int64_t d = 0;
    const int kind = j < p.T ? mux_row(p, j, &d) : 2;   // an idle segment transforms zeros: every barrier, no global memory
    auto ld = [&](int n) -> cx<double> {
        if (kind == 2) return cx<double>{0.0, 0.0};
        const int c = carrier_of_bin(n, p.nf, p.nc);
        if (c < 0) return cx<double>{0.0, 0.0};
        if (kind == 1) return cx<double>{1.0, 0.0};
        const cx<double> v = mem.ld(xrow + 2 * (d * p.nf + c));
        return cx<double>{v.x, -v.y};
    };
    C::first(t, ld, tw, work + sb * C::N);
}

// the group's symbols as ONE run of nsg (nc + ncp) samples: sample m of a symbol is conj(X[(m - ncp) mod nc]) / nc.  complex128: one 16-byte
// store per sample; complex64: aligned pairs, element stores at the run's ends.
template <typename SO, int LOG2N, class Mem>
SK_HD void tx_store(const Mem &mem, const TxPlan &p, SO *yrow, int64_t j0, int tid, const cx<double> *work)
{
    typedef Core<LOG2N> C;
    const int L = p.nc + p.ncp;
    const int64_t left = p.T - j0;
    const int nsg = left < C::NB ? (int)left : C::NB, len = nsg * L;
    const double inv = 1.0 / (double)p.nc;
    SO *run = yrow + 2 * (j0 * L);
    auto get = [&](int e) -> cx<double> {
        const int s = e / L, m = e - s * L;
        int k = m - p.ncp;
        if (k < 0) k += p.nc;
        const cx<double> v = work[s * C::N + C::pos_of(k)];
        return cx<double>{v.x * inv, -v.y * inv};
    };
    if constexpr (sizeof(SO) == 8) {
        for (int e = tid; e < len; e += kThreads) mem.st(run + 2 * e, get(e));
    } else {
        const int h = (int)(((uintptr_t)run >> 3) & 1);   // the run starts in the upper half of a 16-byte unit
        const int nch = (len + h + 1) / 2;
        for (int c = tid; c < nch; c += kThreads) {
            const int ea = 2 * c - h, eb = ea + 1;
            if (ea >= 0 && eb < len) {
                mem.st2(run + 2 * ea, get(ea), get(eb));
            } else {
                if (ea >= 0 && ea < len) mem.st(run + 2 * ea, get(ea));
                if (eb >= 0 && eb < len) mem.st(run + 2 * eb, get(eb));
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------- the receiver
template <typename SI, int LOG2N, class Mem>
SK_HD void rx_first(const Mem &mem, const RxPlan &p, const SI *xrow, int64_t k0, int tid, const cx<double> *tw, cx<double> *work)
{
    typedef Core<LOG2N> C;
    const int sb = tid / C::TS, t = tid % C::TS;
    const int64_t k = k0 + sb;
    const bool active = k < p.nsym;
    const SI *sym = xrow + 2 * (k * p.stride + p.off);
    auto ld = [&](int n) -> cx<double> {
        if (!active) return cx<double>{0.0, 0.0};
        return mem.ld(sym + 2 * n);
    };
    C::first(t, ld, tw, work + sb * C::N);
}

// the nf picked bins of the group's symbols: pilots (npb > 0, k % npb == 0) to pil[k / npb], data to z at their compacted index, divided by
// hht[c] where the divisor is one table for all rows
template <typename SO, int LOG2N, class Mem>
SK_HD void rx_store(const Mem &mem, const RxPlan &p, SO *zrow, double *pil, const cx<double> *hht, int64_t k0, int tid, const cx<double> *work)
{
    typedef Core<LOG2N> C;
    const int64_t left = p.nsym - k0;
    const int nsg = left < C::NB ? (int)left : C::NB, len = nsg * p.nf;
    for (int e = tid; e < len; e += kThreads) {
        const int s = e / p.nf, c = e - s * p.nf;
        const int64_t k = k0 + s;
        cx<double> v = work[s * C::N + C::pos_of(bin_of_carrier(c, p.nf, p.nc))];
        int64_t i = k;
        if (p.npb > 0) {
            const int64_t q = k / p.npb;
            if (k == q * p.npb) {
                mem.st(pil + 2 * (q * p.nf + c), v);
                continue;
            }
            i = k - q - 1;
        }
        if (hht) v = cdiv(v, mem.ld_tab(hht, c));
        mem.st(zrow + 2 * (i * p.nf + c), v);
    }
}

// ---------------------------------------------------------------------------------------------------------------- the estimator
// carrier c of a row: H = z[0], then H = alpha H + (1 - alpha) z[p] over the row's pilots in order (the reference's recursion, float64, no
// contraction); estimate p to est[p], the last one to h.  pilot p is src[p pitch + c]; src may be est (in place).
template <typename SI, class Mem>
SK_HD void chanest_item(const Mem &mem, const SI *src, int64_t pitch, int64_t npilot, int nf, int c, double alpha, double *est, double *h)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double beta = 1.0 - alpha;
    cx<double> H = mem.ld(src + 2 * c);
    mem.st(est + 2 * c, H);
    for (int64_t q = 1; q < npilot; ++q) {
        const cx<double> z = mem.ld(src + 2 * (q * pitch + c));
        H.x = alpha * H.x + beta * z.x;
        H.y = alpha * H.y + beta * z.y;
        mem.st(est + 2 * ((int64_t)q * nf + c), H);
    }
    mem.st(h + 2 * c, H);
}

// element e = i nf + c of a row's data: symbol i + i / (npb - 1) + 1 of src with its pilots in place (compact = 0), or row i of a compacted
// src, divided by hht[c] (the known channel) or by estimate i / (npb - 1)
template <typename SI, typename SO, class Mem>
SK_HD void equalize_item(const Mem &mem, const SI *src, int compact, const double *est, const cx<double> *hht, int nf, int npb, int64_t e, SO *out)
{
    const int64_t i = e / nf, blk = i / (npb - 1);
    const int c = (int)(e - i * nf);
    const int64_t k = compact ? i : i + blk + 1;
    const cx<double> z = mem.ld(src + 2 * (k * nf + c));
    const cx<double> d = hht ? mem.ld_tab(hht, c) : mem.ld(est + 2 * (blk * nf + c));
    mem.st(out + 2 * e, cdiv(z, d));
}

}  // namespace ofdm
}  // namespace skdsp
