// symmap_core.hpp -- the plans, the item geometry and the per-item functions of the Gray symbol mapping kernels behind
// digitalcom.qam_gray_decode / mpsk_gray_decode (digitalcom.py:1684-1739, 1829-1883 of the reference) and the symbol mapping inside
// qam_gray_encode_bb / mpsk_gray_encode_bb (digitalcom.py:1584-1681, 1742-1826).  Plain C++ for host and device: symmap.hip builds its
// kernels from it and tests/host/symmap_emul.cpp walks the same functions thread by thread without a GPU.
//
// Bits travel one byte each (bit 0 significant), MSB first within a symbol's word.  A work item is (row, run of kSymWg symbols); lane t of
// the item takes the fixed set of symbols t, t + kThreads, ... (kSymRun of them): at any input step the 64 lanes of a wave then touch
// adjacent elements.  The item's bits pass through an LDS image laid out by the global run's alignment (blockcode_core.hpp: stage_in /
// stage_out), so every global access to bits is an aligned 16-byte chunk or a byte of the run's head or tail.
//
// Map.  The word of a symbol indexes a table of at most kTab entries that the HOST filled with the reference's own NumPy arithmetic (and,
// for complex64 output, rounded to float32 there): the kernel evaluates no exp, sqrt or division.  QAM of 4 points and more splits the
// word into [I word, Q word] and reads the level table twice; every other plan reads (re, im) of one entry.
//
// Scale (QAM).  np.std of a row is sqrt(M2 / n), M2 = sum |x - mean|^2.  A lane forms (count, mean, M2) of its symbols in two passes over
// its registers, lanes and then work items merge with Chan's update (moments_merge) in a FIXED order: the sum has no atomics, does not
// depend on scheduling, and keeps its accuracy under a DC offset.  r = 1 / (sqrt(M2 / n) c) is what the decision multiplies by.
//
// Decide.  qam_decide is the reference's four steps, each ONE correctly rounded float64 operation in the reference's order (NumPy divides
// a complex array by a real scalar as a multiplication by the rounded reciprocal): no contraction into fused multiply-adds.  mpsk_index is
// angle * mod / 2 / pi in that order, ties to even, reduced by a mask.
#pragma once
#include <math.h>
#include "blockcode_core.hpp"

namespace skdsp {
namespace sym {

constexpr int kThreads = 256;
constexpr int kSymRun = 8;                     // symbols per lane
constexpr int kSymWg = kThreads * kSymRun;     // symbols per work item
constexpr int kMaxBps = 8;                     // bits per symbol: 1, 2, 3, 4, 5, 6 or 8
constexpr int kTab = 32;                       // table entries at most
constexpr int kImgBytes = blk::image_bytes(kMaxBps * kSymWg);
enum Kind { kQam = 0, kMpsk = 1 };

// the order's bits per symbol, 0 for an order the family does not have
inline int bps_of(int kind, int mod)
{
    if (kind == kQam) return mod == 2 ? 1 : mod == 4 ? 2 : mod == 16 ? 4 : mod == 64 ? 6 : mod == 256 ? 8 : 0;
    if (kind == kMpsk) return mod == 2 ? 1 : mod == 4 ? 2 : mod == 8 ? 3 : mod == 16 ? 4 : mod == 32 ? 5 : 0;
    return 0;
}
inline const char *order_check(int kind, int mod)
{
    if (kind != kQam && kind != kMpsk) return "the kind must be 0 (QAM) or 1 (MPSK)";
    if (!bps_of(kind, mod)) return kind == kQam ? "M must be 2, 4, 16, 64, 256" : "M must be 2, 4, 8, 16, or 32";
    return nullptr;
}

struct MapPlan {
    int bps = 0;
    int half = 0;                 // > 0: the word is [I word, Q word] of `half` bits each, both index re[]
    int ntab = 0;
    double re[kTab] = {}, im[kTab] = {};
};
// tab_re / tab_im: ntab entries each, as the host computed them (tab_im is not read where the word is split)
inline const char *map_plan_make(int kind, int mod, const double *tab_re, const double *tab_im, int ntab, MapPlan *p)
{
    const char *why = order_check(kind, mod);
    if (why) return why;
    p->bps = bps_of(kind, mod);
    p->half = (kind == kQam && mod > 2) ? p->bps / 2 : 0;
    p->ntab = 1 << (p->half ? p->half : p->bps);
    if (ntab != p->ntab || !tab_re || (!p->half && !tab_im)) return "the constellation table does not have the order's entries";
    for (int i = 0; i < p->ntab; ++i) {
        p->re[i] = tab_re[i];
        p->im[i] = p->half ? tab_re[i] : tab_im[i];
    }
    return nullptr;
}

struct DemapPlan {
    int kind = 0, mod = 0, bps = 0;
    int x_m = 0;                          // QAM: the top level index, sqrt(mod) - 1 (1 for mod 2)
    double rot_re = 1.0, rot_im = 0.0;    // MPSK, mod 4: the host's np.exp(-1j * pi / 4)
};
inline const char *demap_plan_make(int kind, int mod, double rot_re, double rot_im, DemapPlan *p)
{
    const char *why = order_check(kind, mod);
    if (why) return why;
    p->kind = kind;
    p->mod = mod;
    p->bps = bps_of(kind, mod);
    p->x_m = kind == kQam ? (mod == 2 ? 1 : (1 << (p->bps / 2)) - 1) : 0;
    p->rot_re = rot_re;
    p->rot_im = rot_im;
    return nullptr;
}

// ------------------------------------------------------------------------------------------------------------------ geometry
inline int64_t items_per_row(int64_t n) { return (n + kSymWg - 1) / kSymWg; }
SK_HD int64_t item_first(int64_t it) { return it * kSymWg; }
SK_HD int item_len(int64_t n, int64_t it) { const int64_t left = n - it * kSymWg; return left < kSymWg ? (int)left : kSymWg; }
SK_HD int lane_sym(int t, int u) { return u * kThreads + t; }   // symbol u of lane t within the item

// ------------------------------------------------------------------------------------------------------------------ map
// the MSB-first word of symbol i of an item whose bits are image bytes [lead, lead + bps len)
SK_HD int map_word(const uint8_t *img, int lead, int bps, int i)
{
    int w = 0;
    for (int j = 0; j < bps; ++j) w = (w << 1) | (img[lead + bps * i + j] & 1);
    return w;
}
// the table as the kernel holds it (LDS): the plan's sizes and the two columns
struct MapTab {
    int bps, half;
    const double *re, *im;
};
SK_HD void map_point(const MapTab &p, int w, double *re, double *im)
{
    if (p.half) {
        *re = p.re[w >> p.half];
        *im = p.re[w & ((1 << p.half) - 1)];
    } else {
        *re = p.re[w];
        *im = p.im[w];
    }
}
// Thread t of T stores its share of the item's len symbols at y (the item's first output element).  complex128: one 16-byte store per
// symbol, lanes adjacent.  complex64: 16-byte stores of the symbol pairs that start on a 16-byte boundary, an 8-byte store for the
// (at most one) symbol in front of the first pair and behind the last.  Mem: st_c128(double *, re, im), st_c64(float *, re, im),
// st_c64x2(float *, re0, im0, re1, im1).
template <class Mem> SK_HD void map_store(const Mem &m, const MapTab &p, const uint8_t *img, int lead, int len, void *y, int c64, int t, int T)
{
    double re, im;
    if (!c64) {
        double *g = static_cast<double *>(y);
        for (int i = t; i < len; i += T) {
            map_point(p, map_word(img, lead, p.bps, i), &re, &im);
            m.st_c128(g + 2 * (int64_t)i, re, im);
        }
        return;
    }
    float *g = static_cast<float *>(y);
    const int head = (int)(((uintptr_t)y >> 3) & 1), npair = (len - head) / 2;
    for (int q = t; q < npair; q += T) {
        const int i = head + 2 * q;
        double re1, im1;
        map_point(p, map_word(img, lead, p.bps, i), &re, &im);
        map_point(p, map_word(img, lead, p.bps, i + 1), &re1, &im1);
        m.st_c64x2(g + 2 * (int64_t)i, (float)re, (float)im, (float)re1, (float)im1);
    }
    const int tail = head + 2 * npair;   // < len: one symbol behind the last pair
    if (t == 0 && head && len > 0) {
        map_point(p, map_word(img, lead, p.bps, 0), &re, &im);
        m.st_c64(g, (float)re, (float)im);
    }
    if (t == (T > 1 ? 1 : 0) && tail < len) {
        map_point(p, map_word(img, lead, p.bps, tail), &re, &im);
        m.st_c64(g + 2 * (int64_t)tail, (float)re, (float)im);
    }
}

// ------------------------------------------------------------------------------------------------------------------ scale
struct Moments {
    double n, mre, mim, m2;   // count, mean, sum |x - mean|^2
};
SK_HD Moments moments_none() { return Moments{0.0, 0.0, 0.0, 0.0}; }
// the moments of cnt values held in registers: mean first, then the squared distances from it
SK_HD Moments moments_lane(const double *re, const double *im, int cnt)
{
    Moments a = moments_none();
    if (cnt <= 0) return a;
    double sr = 0.0, si = 0.0;
    for (int j = 0; j < cnt; ++j) {
        sr += re[j];
        si += im[j];
    }
    a.n = (double)cnt;
    a.mre = sr / a.n;
    a.mim = si / a.n;
    for (int j = 0; j < cnt; ++j) {
        const double dr = re[j] - a.mre, di = im[j] - a.mim;
        a.m2 += dr * dr + di * di;
    }
    return a;
}
// Chan, Golub, LeVeque: the moments of the union of two disjoint sets
SK_HD Moments moments_merge(const Moments &a, const Moments &b)
{
    if (b.n == 0.0) return a;
    if (a.n == 0.0) return b;
    Moments c;
    c.n = a.n + b.n;
    const double dr = b.mre - a.mre, di = b.mim - a.mim, f = b.n / c.n;
    c.mre = a.mre + dr * f;
    c.mim = a.mim + di * f;
    c.m2 = a.m2 + b.m2 + (dr * dr + di * di) * (a.n * f);
    return c;
}
// the tree over the T slots of a workgroup (T a power of two): after step `off`, slot t < off holds the merge of t and t + off.  The
// caller runs the steps off = T / 2 ... 1 with a barrier between them; merge_step is one thread's part of one step.
SK_HD void merge_step(Moments *slot, int off, int t)
{
    if (t < off) slot[t] = moments_merge(slot[t], slot[t + off]);
}
// what thread t of T merges, in order, when a row's `items` partials are dealt in contiguous shares
SK_HD void share_of(int64_t items, int t, int T, int64_t *lo, int64_t *hi)
{
    const int64_t per = (items + T - 1) / T;
    *lo = per * t < items ? per * t : items;
    *hi = *lo + per < items ? *lo + per : items;
}
// r = 1 / (np.std(row) c): the reference's sqrt, product and reciprocal in its order
SK_HD double scale_of(const Moments &a, double c) { return 1.0 / (sqrt(a.m2 / a.n) * c); }

// ------------------------------------------------------------------------------------------------------------------ decide
#if defined(__clang__)
#define SK_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define SK_NO_CONTRACT   // (a host compiler other than clang: build with -ffp-contract=off, as the tests do)
#endif
// one component: int16(clip(rint((v r + x_m) / 2), 0, x_m)), r = 1.0 / s
SK_HD int qam_level(double v, double r, int x_m)
{
    SK_NO_CONTRACT
    const double scaled = v * r;
    const double shifted = scaled + (double)x_m;
    const double k = rint(shifted * 0.5);
    if (!(k > 0.0)) return 0;   // (also what is not a number: the reference's cast of it is platform-defined)
    return k > (double)x_m ? x_m : (int)k;
}
SK_HD void qam_decide(double re, double im, double r, int x_m, int *kI, int *kQ)
{
    *kI = qam_level(re, r, x_m);
    *kQ = qam_level(im, r, x_m);
}
// ---- atan2 rounded to nearest, from + - * / and fma alone.  The decision rint(angle * mod / 2 / pi) sits on a tie for inputs a user can type
// (1, 1j, ... under the QPSK rotation), where one ulp of the angle decides the symbol: the reference's libm rounds its atan2 correctly there,
// a device library's (2 ulp) need not, and host and device must agree to the bit.  So the angle is built in double-double: the octant
// folded to alpha = atan(lo / hi) in [0, pi / 4], alpha = k pi / 16 + atan(u) with u = (lo c_k - hi s_k) / (hi c_k + lo s_k), |u| <= tan(pi / 32)
// (the rotation by -k pi / 16 with c_k, s_k as double-double constants: tools/gen_symmap_atan_table.py), atan(u) = u - u^3 / 3 + ... with the
// leading term in double-double, then pi / 2 - alpha and pi - . as the octant asks.  The error is about 1e-19: below half an ulp of every
// result but for angles within 1e-19 of the midpoint of two doubles.
struct DD {
    double h, l;
};
SK_HD DD two_sum(double a, double b)
{
    SK_NO_CONTRACT
    const double s = a + b, bb = s - a;
    return DD{s, (a - (s - bb)) + (b - bb)};
}
SK_HD DD two_prod(double a, double b)
{
    SK_NO_CONTRACT
    const double p = a * b;
    return DD{p, fma(a, b, -p)};
}
// a c +- b d for doubles a, b and double-double constants c, d
SK_HD DD dd_dot(double a, DD c, double b, DD d, double sign)
{
    SK_NO_CONTRACT
    const DD p = two_prod(a, c.h), q = two_prod(b, d.h);
    const DD s = two_sum(p.h, sign * q.h);
    const double low = s.l + (p.l + sign * q.l) + (a * c.l + sign * (b * d.l));
    return two_sum(s.h, low);
}
SK_HD DD dd_sub(DD a, DD b)
{
    SK_NO_CONTRACT
    const DD s = two_sum(a.h, -b.h);
    return two_sum(s.h, s.l + (a.l - b.l));
}
SK_HD double atan2_rn(double y, double x)
{
    SK_NO_CONTRACT
    const double pi = 0x1.921fb54442d18p+1;
    if (y == 0.0) return copysign(signbit(x) ? pi : 0.0, y);     // IEEE's exact values on the axes
    if (x == 0.0) return copysign(0.5 * pi, y);
    double ax = fabs(x), ay = fabs(y);
    const bool swap = ay > ax;
    double hi = swap ? ay : ax, lo = swap ? ax : ay;
    if (hi > 0x1p+1000) {            // keep hi (c + s) finite and lo normal: powers of two, exact
        hi *= 0x1p-200;
        lo *= 0x1p-200;
    } else if (hi < 0x1p-900) {
        hi *= 0x1p+200;
        lo *= 0x1p+200;
    }
    const double q = lo / hi;
    const int k = q < 0x1.936bb8c5b2da2p-4 ? 0 : q < 0x1.36a08355c63dcp-2 ? 1 : q < 0x1.11ab7190834ecp-1 ? 2 : q < 0x1.a43002ae42850p-1 ? 3 : 4;
    // k pi / 16, cos and sin of it, (hi, lo) each
    DD a, c, s;
    switch (k) {
    case 0: a = DD{0.0, 0.0}; c = DD{1.0, 0.0}; s = DD{0.0, 0.0}; break;
    case 1: a = DD{0x1.921fb54442d18p-3, 0x1.1a62633145c07p-57}; c = DD{0x1.f6297cff75cb0p-1, 0x1.562172a361fd3p-56}; s = DD{0x1.8f8b83c69a60bp-3, -0x1.26d19b9ff8d82p-57}; break;
    case 2: a = DD{0x1.921fb54442d18p-2, 0x1.1a62633145c07p-56}; c = DD{0x1.d906bcf328d46p-1, 0x1.457e610231ac2p-56}; s = DD{0x1.87de2a6aea963p-2, -0x1.72cedd3d5a610p-57}; break;
    case 3: a = DD{0x1.2d97c7f3321d2p-1, 0x1.a79394c9e8a0ap-56}; c = DD{0x1.a9b66290ea1a3p-1, 0x1.9f630e8b6dac8p-60}; s = DD{0x1.1c73b39ae68c8p-1, 0x1.b25dd267f6600p-55}; break;
    default: a = DD{0x1.921fb54442d18p-1, 0x1.1a62633145c07p-55}; c = DD{0x1.6a09e667f3bcdp-1, -0x1.bdd3413b26456p-55}; s = DD{0x1.6a09e667f3bcdp-1, -0x1.bdd3413b26456p-55}; break;
    }
    const DD num = dd_dot(lo, c, hi, s, -1.0), den = dd_dot(hi, c, lo, s, 1.0);
    const double u = num.h / den.h;
    const double rem = fma(-u, den.h, num.h);                    // exact
    const double u2 = u * u;
    const double ul = ((rem + num.l) - u * den.l) / den.h / (1.0 + u2);   // the quotient's second word, carried through atan'(u)
    double t = -1.0 / 19.0;
    t = t * u2 + 1.0 / 17.0;
    t = t * u2 - 1.0 / 15.0;
    t = t * u2 + 1.0 / 13.0;
    t = t * u2 - 1.0 / 11.0;
    t = t * u2 + 1.0 / 9.0;
    t = t * u2 - 1.0 / 7.0;
    t = t * u2 + 1.0 / 5.0;
    t = t * u2 - 1.0 / 3.0;
    const double tail = t * u2 * u;                              // atan(u) - u
    const DD s1 = two_sum(a.h, u);
    DD ang = two_sum(s1.h, s1.l + (a.l + ul + tail));
    if (swap) ang = dd_sub(DD{0x1.921fb54442d18p+0, 0x1.1a62633145c07p-54}, ang);
    if (signbit(x)) ang = dd_sub(DD{0x1.921fb54442d18p+1, 0x1.1a62633145c07p-53}, ang);
    return copysign(ang.h, y);
}

// np.mod(rint(angle(x [exp(-1j pi / 4)]) * mod / 2 / pi), mod), in the reference's order of operations
SK_HD int mpsk_index(double re, double im, const DemapPlan &p)
{
    SK_NO_CONTRACT
    if (p.mod == 4) {
        const double a = re * p.rot_re, b = im * p.rot_im, c = re * p.rot_im, d = im * p.rot_re;
        re = a - b;
        im = c + d;
    }
    const double pi = 0x1.921fb54442d18p+1;
    const double ang = atan2_rn(im, re);
    const double scaled = ang * (double)p.mod;
    const double k = rint(scaled / 2.0 / pi);
    if (!(k == k)) return 0;
    return (int)((long long)k & (long long)(p.mod - 1));
}
// the symbol's bits as a word, MSB first: Gray v ^ (v >> 1) of each level index (QAM: [I word, Q word])
SK_HD int qam_bits(const DemapPlan &p, int kI, int kQ)
{
    if (p.mod == 2) return kI;
    return ((kI ^ (kI >> 1)) << (p.bps / 2)) | (kQ ^ (kQ >> 1));
}
SK_HD int mpsk_bits(int idx) { return idx ^ (idx >> 1); }
SK_HD void put_bits(uint8_t *img, int at, int bps, int word)
{
    for (int j = 0; j < bps; ++j) img[at + j] = (uint8_t)((word >> (bps - 1 - j)) & 1);
}

// Element e of a row of complex64 (c64) or complex128 values, widened exactly.  Mem: ld_c64(const float *, &re, &im), ld_c128(const double *, ...)
template <class Mem> SK_HD void load_sym(const Mem &m, const void *row, int64_t e, int c64, double *re, double *im)
{
    if (c64) m.ld_c64(static_cast<const float *>(row) + 2 * e, re, im);
    else m.ld_c128(static_cast<const double *>(row) + 2 * e, re, im);
}
// lane t's moments of the item's len symbols; sym0: the element of the item's first symbol, step: elements from symbol to symbol
template <class Mem> SK_HD Moments scale_lane(const Mem &m, const void *row, int64_t sym0, int64_t step, int c64, int len, int t)
{
    double re[kSymRun], im[kSymRun];
    int cnt = 0;
    for (int u = 0; u < kSymRun; ++u) {
        const int i = lane_sym(t, u);
        if (i < len) {
            load_sym(m, row, sym0 + i * step, c64, &re[cnt], &im[cnt]);
            ++cnt;
        }
    }
    return moments_lane(re, im, cnt);
}
// the same over a row of REAL values, float32 (f32) or float64, each a symbol on the real axis (the channel's np.var of a real signal):
// element sym0 + i step.  Mem: ld_f32(const float *), ld_f64(const double *), the value widened exactly
template <class Mem> SK_HD Moments scale_lane_real(const Mem &m, const void *row, int64_t sym0, int64_t step, int f32, int len, int t)
{
    double re[kSymRun], im[kSymRun];
    int cnt = 0;
    for (int u = 0; u < kSymRun; ++u) {
        const int i = lane_sym(t, u);
        if (i < len) {
            const int64_t e = sym0 + i * step;
            re[cnt] = f32 ? m.ld_f32(static_cast<const float *>(row) + e) : m.ld_f64(static_cast<const double *>(row) + e);
            im[cnt] = 0.0;
            ++cnt;
        }
    }
    return moments_lane(re, im, cnt);
}
// np.var of the merged row: M2 / n
SK_HD double var_of(const Moments &a) { return a.m2 / a.n; }
// lane t's symbols of the item decided into the output image (the item's bits at image bytes [lead, lead + bps len))
template <class Mem> SK_HD void demap_lane(const Mem &m, const DemapPlan &p, const void *row, int64_t sym0, int64_t step, int c64, int len, double r, uint8_t *img, int lead, int t)
{
    for (int u = 0; u < kSymRun; ++u) {
        const int i = lane_sym(t, u);
        if (i >= len) break;
        double re, im;
        load_sym(m, row, sym0 + i * step, c64, &re, &im);
        int word;
        if (p.kind == kQam) {
            int kI, kQ;
            qam_decide(re, im, r, p.x_m, &kI, &kQ);
            word = qam_bits(p, kI, kQ);
        } else {
            word = mpsk_bits(mpsk_index(re, im, p));
        }
        put_bits(img, lead + p.bps * i, p.bps, word);
    }
}

}  // namespace sym
}  // namespace skdsp
