// channel_core.hpp -- the draw, the plans, the chunk geometry and the per-chunk functions of the channel and source kernels behind
// sigsys.cpx_awgn / cpx_awgn2 (sigsys.py:2335-2454 of the reference), digitalcom.awgn_channel (digitalcom.py:1259-1281), sigsys.pn_gen / m_seq
// (sigsys.py:1947-2050) and the random data bits of the BER loops.  Plain C++ for host and device: channel.hip builds its kernels from it and
// tests/host/channel_emul.cpp walks the same functions thread by thread without a GPU.
//
// The draw.  Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11) with key = the 64-bit seed and
// counter = (block lo, block hi, row, tag): tag 0 normals, tag 1 bits.  One block of tag 0 is one complex normal: u1 = (k1 + 1) 2^-53 in
// (0, 1] from the top 53 bits of words 0, 1 and u2 = k2 2^-53 in [0, 1) from words 2, 3, z = sqrt(-2 ln u1) (cos 2 pi u2 + j sin 2 pi u2).
// A REAL stream's element i is component i & 1 of block i >> 1, so a complex stream is the real stream of twice the index: every kernel
// walks one "component stream" q.  One block of tag 1 is 128 bits: bit k of the block is bit k & 31 of word k >> 5.
//
// ln and sincos are this file's own, float64 + - * / only with contraction off and no fma, in ONE fixed order: the NumPy restatement
// (_ffi.normals_host) performs the same operations and gets the same bits.  ln u1 = e ln 2 + 2 atanh((m - 1) / (m + 1)) over
// m in [sqrt(1/2), sqrt(2)) (u1 -> 1 keeps e = 0 and m - 1 exact: no cancellation); 2 pi u2 is reduced EXACTLY on the integer k2 (the top
// three bits are the octant, odd octants mirror the remaining 50), the sine and cosine of x in [0, pi / 4] are Taylor polynomials.
//
// Geometry.  A row's output run is cut into the aligned 16-byte chunks of memory that it touches.  A work item is (row, kChunksWg chunks);
// thread t takes chunks t, t + kThreads, ...: adjacent lanes, adjacent chunks.  A chunk inside the run leaves as one 16-byte store, the
// components (bytes for the bit kernels) of the at most two partial chunks at the run's ends leave one by one, nothing else is touched.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>
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
namespace chan {

constexpr int kThreads = 256;
constexpr int kChunkRun = 4;                        // chunks per lane
constexpr int kChunksWg = kThreads * kChunkRun;     // chunks per work item: 16 KiB of output
enum Tag { kTagNormal = 0, kTagBits = 1 };
enum SigmaMode { kSigmaAwgn = 0, kSigmaAwgn2 = 1 };

// ------------------------------------------------------------------------------------------------------------------ Philox4x32-10
struct Block {
    uint32_t w[4];
};
SK_HD Block philox(uint64_t seed, uint64_t blk, uint32_t row, uint32_t tag)
{
    uint32_t c0 = (uint32_t)blk, c1 = (uint32_t)(blk >> 32), c2 = row, c3 = tag;
    uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1;
        c3 = (uint32_t)p0;
        c0 = n0;
        c2 = n2;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return Block{{c0, c1, c2, c3}};
}
// the block function on a free counter and key: what the known-answer vectors are stated on
SK_HD Block philox_raw(const uint32_t ctr[4], const uint32_t key[2])
{
    return philox((uint64_t)key[0] | ((uint64_t)key[1] << 32), (uint64_t)ctr[0] | ((uint64_t)ctr[1] << 32), ctr[2], ctr[3]);
}

// ------------------------------------------------------------------------------------------------------------------ ln, sincos
SK_HD double bits_to_double(uint64_t b)
{
    double d;
    memcpy(&d, &b, 8);
    return d;
}
SK_HD uint64_t double_to_bits(double d)
{
    uint64_t b;
    memcpy(&b, &d, 8);
    return b;
}
// -ln(k 2^-53), k = 1 ... 2^53
SK_HD double neg_ln_u(uint64_t k)
{
    SK_NO_CONTRACT
    const uint64_t b = double_to_bits((double)k);                 // exact: k <= 2^53
    int e = (int)(b >> 52) - 1023 - 53;                           // u = m 2^e, m in [1, 2)
    double m = bits_to_double((b & 0x000fffffffffffffull) | 0x3ff0000000000000ull);
    if (m >= 0x1.6a09e667f3bcdp+0) {                              // m in [sqrt(1/2), sqrt(2))
        m = m * 0.5;
        e += 1;
    }
    const double s = (m - 1.0) / (m + 1.0);
    const double z = s * s;
    double p = 1.0 / 25.0;
    p = p * z + 1.0 / 23.0;
    p = p * z + 1.0 / 21.0;
    p = p * z + 1.0 / 19.0;
    p = p * z + 1.0 / 17.0;
    p = p * z + 1.0 / 15.0;
    p = p * z + 1.0 / 13.0;
    p = p * z + 1.0 / 11.0;
    p = p * z + 1.0 / 9.0;
    p = p * z + 1.0 / 7.0;
    p = p * z + 1.0 / 5.0;
    p = p * z + 1.0 / 3.0;
    const double lnm = 2.0 * s + 2.0 * s * (z * p);              // 2 atanh(s)
    const double ne = (double)(-e);                               // 0 ... 53
    // ln 2 = hi + lo, hi of 32 significant bits: ne hi is exact
    return ne * 0x1.62e42feep-1 + (ne * 0x1.a39ef35793c76p-33 - lnm);
}
// the polynomial stage: sin and cos of x in [0, pi / 4] (shared with carrier_core.hpp's sincos_rad, which reduces an angle in radians to it)
SK_HD void sincos_octant(double x, double *sin_x, double *cos_x)
{
    SK_NO_CONTRACT
    const double z = x * x;
    double ps = 1.0 / 355687428096000.0;                          // 1 / 17!
    ps = -1.0 / 1307674368000.0 + z * ps;                         // 15!
    ps = 1.0 / 6227020800.0 + z * ps;                             // 13!
    ps = -1.0 / 39916800.0 + z * ps;                              // 11!
    ps = 1.0 / 362880.0 + z * ps;                                 // 9!
    ps = -1.0 / 5040.0 + z * ps;                                  // 7!
    ps = 1.0 / 120.0 + z * ps;                                    // 5!
    ps = -1.0 / 6.0 + z * ps;                                     // 3!
    const double sx = x + x * (z * ps);
    double pc = -1.0 / 6402373705728000.0;                        // 1 / 18!
    pc = 1.0 / 20922789888000.0 + z * pc;                         // 16!
    pc = -1.0 / 87178291200.0 + z * pc;                           // 14!
    pc = 1.0 / 479001600.0 + z * pc;                              // 12!
    pc = -1.0 / 3628800.0 + z * pc;                               // 10!
    pc = 1.0 / 40320.0 + z * pc;                                  // 8!
    pc = -1.0 / 720.0 + z * pc;                                   // 6!
    pc = 1.0 / 24.0 + z * pc;                                     // 4!
    *sin_x = sx;
    *cos_x = 1.0 - (0.5 * z - (z * z) * pc);
}
// cos and sin of 2 pi k 2^-53, k = 0 ... 2^53 - 1
SK_HD void sincos_2pi(uint64_t k, double *c, double *s)
{
    SK_NO_CONTRACT
    const int oct = (int)(k >> 50);
    uint64_t f = k & (((uint64_t)1 << 50) - 1);
    if (oct & 1) f = ((uint64_t)1 << 50) - f;                    // the mirror image within the octant: exact
    const double x = ((double)f * 0x1p-53) * 0x1.921fb54442d18p+2;   // 2 pi t, t in [0, 1 / 8]
    double sx, cx;
    sincos_octant(x, &sx, &cx);
    const bool sw =((oct + 1) & 2) != 0;                         // octants 1, 2, 5, 6: the angle is measured from the imaginary axis
    const double ca = sw ? sx : cx, sa = sw ? cx : sx;
    *c = ((oct + 2) & 4) ? -ca : ca;                              // octants 2 ... 5: the left half plane
    *s = (oct & 4) ? -sa : sa;                                    // octants 4 ... 7: the lower
}
// sqrt is one correctly rounded IEEE operation on the host and, as the device / host comparison of the tests confirms, on the device
SK_HD double sqrt_rn(double a) { return sqrt(a); }

// the complex normal of a block of tag 0
SK_HD void normal_of(const Block &b, double *re, double *im)
{
    SK_NO_CONTRACT
    const uint64_t k1 = ((uint64_t)b.w[0] << 21) | (b.w[1] >> 11), k2 = ((uint64_t)b.w[2] << 21) | (b.w[3] >> 11);
    const double r = sqrt_rn(2.0 * neg_ln_u(k1 + 1));
    double c, s;
    sincos_2pi(k2, &c, &s);
    *re = r * c;
    *im = r * s;
}
SK_HD void normal_block(uint64_t seed, uint32_t row, uint64_t blk, double *re, double *im) { normal_of(philox(seed, blk, row, kTagNormal), re, im); }
// bit k (0 ... 127) of a block of tag 1
SK_HD uint32_t bit_of(const Block &b, int k)
{
    const int j = k >> 5;
    const uint32_t w = j == 0 ? b.w[0] : j == 1 ? b.w[1] : j == 2 ? b.w[2] : b.w[3];
    return (w >> (k & 31)) & 1u;
}

// ------------------------------------------------------------------------------------------------------------------ geometry
// the work items that cover the chunks a run of `bytes` bytes can touch: whatever its alignment, or (aligned16) where every row of the call
// starts on a 16-byte boundary
inline int64_t items_per_row(int64_t bytes, bool aligned16) { return bytes <= 0 ? 0 : ((bytes + (aligned16 ? 15 : 30)) / 16 + kChunksWg - 1) / kChunksWg; }
inline bool rows_aligned16(const void *y, int64_t stride_bytes) { return (((uintptr_t)y | (uintptr_t)stride_bytes) & 15) == 0; }
SK_HD int lead_of(const void *g) { return (int)((uintptr_t)g & 15); }
SK_HD int64_t lane_chunk(int64_t it, int t, int u) { return it * kChunksWg + (int64_t)u * kThreads + t; }

// ------------------------------------------------------------------------------------------------------------------ awgn
// y = g x + sigma z over component streams: the dtype codes are the library's (0 float32, 1 complex64, 2 float64, 3 complex128)
struct AwgnPlan {
    int y_f32 = 0, y_cpx = 0, x_cpx = 0;   // component size and layout of y; x has y's precision, and y's layout or (x_cpx = 0) real
    uint64_t seed = 0;
    int64_t first = 0;                     // stream index of element 0 of a row
    uint32_t first_row = 0;
    int64_t n = 0;                         // elements per row
};
inline const char *awgn_plan_make(int x_dtype, int y_dtype, uint64_t seed, int64_t first, int64_t first_row, int64_t n, AwgnPlan *p)
{
    if (x_dtype < 0 || x_dtype > 3 || y_dtype < 0 || y_dtype > 3) return "float32, complex64, float64 or complex128 signals";
    if ((x_dtype >> 1) != (y_dtype >> 1)) return "x and y must have the same precision";
    if ((x_dtype & 1) && !(y_dtype & 1)) return "a complex x needs a complex y";
    if (first < 0 || first_row < 0 || n < 0 || first >= ((int64_t)1 << 61) || n >= ((int64_t)1 << 40) || first_row > 0xffffffffll)
        return "need 0 <= first_index < 2^61, 0 <= first_row < 2^32, 0 <= n < 2^40";
    p->y_f32 = (y_dtype >> 1) == 0;
    p->y_cpx = y_dtype & 1;
    p->x_cpx = x_dtype & 1;
    p->seed = seed;
    p->first = first;
    p->first_row = (uint32_t)first_row;
    p->n = n;
    return nullptr;
}
SK_HD int awgn_comp_bytes(const AwgnPlan &p) { return p.y_f32 ? 4 : 8; }
SK_HD int64_t awgn_row_bytes(const AwgnPlan &p) { return p.n * awgn_comp_bytes(p) * (p.y_cpx ? 2 : 1); }

// z[k] = the normal of component-stream position q0 + k of a row for the slots a <= k < b (of 4): each block is drawn once
SK_HD void normals_run(uint64_t seed, uint32_t row, int64_t q0, int a, int b, double *z)
{
    if (a >= b) return;
    const int64_t b0 = (q0 + a) >> 1, b1 = (q0 + b - 1) >> 1;
    for (int64_t blk = b0; blk <= b1; ++blk) {
        double re, im;
        normal_block(seed, row, (uint64_t)blk, &re, &im);
        SK_UNROLL
        for (int k = 0; k < 4; ++k)
            if (k >= a && k < b && ((q0 + k) >> 1) == blk) z[k] = ((q0 + k) & 1) ? im : re;
    }
}
SK_HD double awgn_value(double g, double x, double sigma, double z, bool has_x)
{
    SK_NO_CONTRACT
    const double a = has_x ? g * x : 0.0, w = sigma * z;
    return a + w;
}
// Chunk c of row `row`.  y / x: the row's first component; Mem: ld_f32 / ld_f64 (one component, widened), st_f32 / st_f64, ld_f32x4 /
// ld_f64x2 and st_f32x4 / st_f64x2 (16 bytes at a multiple of 16).
template <class Mem> SK_HD void awgn_chunk(const Mem &m, const AwgnPlan &p, uint32_t row, const void *x, void *y, double g, double sigma, int64_t c)
{
    const int cs = awgn_comp_bytes(p), per = 16 / cs;              // components per chunk: 4 or 2
    const int lead = lead_of(y);                                    // (a multiple of cs: y is aligned to its element)
    const int64_t bytes = awgn_row_bytes(p), lo = 16 * c - lead;   // the chunk's first byte as an offset into the run
    if (lo + 16 <= 0 || lo >= bytes) return;
    const bool full = lo >= 0 && lo + 16 <= bytes;
    const int64_t k0 = lo / cs, ncomp = bytes / cs;                 // the component of the chunk's slot 0 (negative in the head chunk)
    const int64_t q0 = (p.y_cpx ? 2 : 1) * p.first + k0;
    const int a = k0 < 0 ? (int)-k0 : 0, b = k0 + per > ncomp ? (int)(ncomp - k0) : per;   // the slots that are components of the run
    double z[4] = {0.0, 0.0, 0.0, 0.0}, xv[4] = {0.0, 0.0, 0.0, 0.0};
    normals_run(p.seed, p.first_row + row, q0, a, b, z);
    const bool same = p.x_cpx == p.y_cpx;
    if (p.y_f32) {
        const float *xf = static_cast<const float *>(x);
        float *yf = static_cast<float *>(y);
        if (full && same && lead_of(xf + k0) == 0) {
            m.ld_f32x4(xf + k0, xv);
        } else {
            SK_UNROLL
            for (int k = 0; k < 4; ++k) {
                if (k < a || k >= b) continue;
                if (same) xv[k] = m.ld_f32(xf + k0 + k);
                else if (!((k0 + k) & 1)) xv[k] = m.ld_f32(xf + ((k0 + k) >> 1));
            }
        }
        float o[4];
        SK_UNROLL
        for (int k = 0; k < 4; ++k) o[k] = (float)awgn_value(g, xv[k], sigma, z[k], same || !((k0 + k) & 1));
        if (full) {
            m.st_f32x4(yf + k0, o[0], o[1], o[2], o[3]);
        } else {
            SK_UNROLL
            for (int k = 0; k < 4; ++k)
                if (k >= a && k < b) m.st_f32(yf + k0 + k, o[k]);
        }
    } else {
        const double *xd = static_cast<const double *>(x);
        double *yd = static_cast<double *>(y);
        if (full && same && lead_of(xd + k0) == 0) {
            m.ld_f64x2(xd + k0, xv);
        } else {
            SK_UNROLL
            for (int k = 0; k < 2; ++k) {
                if (k < a || k >= b) continue;
                if (same) xv[k] = m.ld_f64(xd + k0 + k);
                else if (!((k0 + k) & 1)) xv[k] = m.ld_f64(xd + ((k0 + k) >> 1));
            }
        }
        double o[2];
        SK_UNROLL
        for (int k = 0; k < 2; ++k) o[k] = awgn_value(g, xv[k], sigma, z[k], same || !((k0 + k) & 1));
        if (full) {
            m.st_f64x2(yd + k0, o[0], o[1]);
        } else {
            SK_UNROLL
            for (int k = 0; k < 2; ++k)
                if (k >= a && k < b) m.st_f64(yd + k0 + k, o[k]);
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------ the bit kernels
// 16 bytes of a chunk as four words, byte j of the chunk in bits 8 (j & 3) ... of word j >> 2
struct Bytes16 {
    uint32_t w[4];
};
SK_HD void put_byte(Bytes16 &v, int j, uint32_t byte) { v.w[j >> 2] |= byte << (8 * (j & 3)); }
SK_HD uint32_t get_byte(const Bytes16 &v, int j) { return (v.w[j >> 2] >> (8 * (j & 3))) & 0xffu; }
// A chunk of a byte run [g, g + n): a, b = the chunk's bytes that belong to the run, *e0 = the run offset of its byte 0 (negative in the head)
SK_HD bool byte_chunk(const void *g, int64_t n, int64_t c, int64_t *e0, int *a, int *b)
{
    const int64_t lo = 16 * c - lead_of(g);
    if (lo + 16 <= 0 || lo >= n) return false;
    *e0 = lo;
    *a = lo < 0 ? (int)-lo : 0;
    *b = lo + 16 > n ? (int)(n - lo) : 16;
    return true;
}
// Mem: ld8 / st8, ld_b16 / st_b16 (16 bytes at a multiple of 16 to / from a Bytes16)
template <class Mem> SK_HD void store_chunk(const Mem &m, uint8_t *g, int64_t e0, int a, int b, const Bytes16 &v)
{
    if (a == 0 && b == 16) {
        m.st_b16(g + e0, v);
        return;
    }
SK_UNROLL
    for (int j = 0; j < 16; ++j)
        if (j >= a && j < b) m.st8(g + e0 + j, (uint8_t)get_byte(v, j));
}

struct BitsPlan {
    uint64_t seed = 0;
    int64_t first = 0, n = 0;
    uint32_t first_row = 0;
};
inline const char *bits_plan_make(uint64_t seed, int64_t first, int64_t first_row, int64_t n, BitsPlan *p)
{
    if (first < 0 || first_row < 0 || n < 0 || first >= ((int64_t)1 << 61) || n >= ((int64_t)1 << 40) || first_row > 0xffffffffll)
        return "need 0 <= first_index < 2^61, 0 <= first_row < 2^32, 0 <= n < 2^40";
    p->seed = seed;
    p->first = first;
    p->first_row = (uint32_t)first_row;
    p->n = n;
    return nullptr;
}
// random bits: chunk c of the row whose output run starts at out
template <class Mem> SK_HD void randbits_chunk(const Mem &m, const BitsPlan &p, uint32_t row, uint8_t *out, int64_t c)
{
    int64_t e0;
    int a, b;
    if (!byte_chunk(out, p.n, c, &e0, &a, &b)) return;
    const int64_t q0 = p.first + e0 + a, q1 = p.first + e0 + b - 1;   // the stream's bits of this chunk
    Bytes16 v = {{0, 0, 0, 0}};
    for (int64_t blk = q0 >> 7; blk <= (q1 >> 7); ++blk) {             // one block, two where the chunk straddles a multiple of 128
        const Block w = philox(p.seed, (uint64_t)blk, p.first_row + row, kTagBits);
SK_UNROLL
        for (int j = 0; j < 16; ++j) {
            const int64_t q = p.first + e0 + j;
            if (j >= a && j < b && (q >> 7) == blk) put_byte(v, j, bit_of(w, (int)(q & 127)));
        }
    }
    store_chunk(m, out, e0, a, b, v);
}
// the hard decision of a bit through the channel: 1 / 0 by the sign of 2 b - 1 + sigma z, 2 for an exact zero, 3 for what is not a number
SK_HD uint32_t awgn_bit(uint32_t bit, double sigma, double z)
{
    SK_NO_CONTRACT
    const double w = sigma * z;
    const double v = (double)(2 * (int)(bit & 1u) - 1) + w;
    return v > 0.0 ? 1u : v < 0.0 ? 0u : v == 0.0 ? 2u : 3u;
}
template <class Mem> SK_HD void awgn_bits_chunk(const Mem &m, const BitsPlan &p, uint32_t row, const uint8_t *in, uint8_t *out, double sigma, int64_t c)
{
    int64_t e0;
    int a, b;
    if (!byte_chunk(out, p.n, c, &e0, &a, &b)) return;
    Bytes16 x = {{0, 0, 0, 0}}, v = {{0, 0, 0, 0}};
    if (a == 0 && b == 16 && lead_of(in + e0) == 0) {
        m.ld_b16(in + e0, x);
    } else {
SK_UNROLL
        for (int j = 0; j < 16; ++j)
            if (j >= a && j < b) put_byte(x, j, m.ld8(in + e0 + j));
    }
    for (int h = 0; h < 4; ++h) {                                      // four bytes at a time: the normals of a word
        const int ja = a - 4 * h < 0 ? 0 : a - 4 * h, jb = b - 4 * h > 4 ? 4 : b - 4 * h;   // the word's bytes that belong to the run
        if (ja >= jb) continue;
        double z[4] = {0.0, 0.0, 0.0, 0.0};
        normals_run(p.seed, p.first_row + row, p.first + e0 + 4 * h, ja, jb, z);
        const uint32_t xw = h == 0 ? x.w[0] : h == 1 ? x.w[1] : h == 2 ? x.w[2] : x.w[3];
        uint32_t word = 0;
        SK_UNROLL
        for (int k = 0; k < 4; ++k)
            if (k >= ja && k < jb) word |= awgn_bit((xw >> (8 * k)) & 0xffu, sigma, z[k]) << (8 * k);
        if (h == 0) v.w[0] = word;
        else if (h == 1) v.w[1] = word;
        else if (h == 2) v.w[2] = word;
        else v.w[3] = word;
    }
    store_chunk(m, out, e0, a, b, v);
}

// ------------------------------------------------------------------------------------------------------------------ periodic sequences
struct PnPlan {
    int64_t first = 0, n = 0;
    int Q = 0;
};
inline const char *pn_plan_make(int Q, int64_t first, int64_t n, PnPlan *p)
{
    if (Q < 1 || Q > 65535) return "the period must be 1 ... 65535 bytes";
    if (first < 0 || n < 0 || first >= ((int64_t)1 << 61) || n >= ((int64_t)1 << 40)) return "need 0 <= first_index < 2^61, 0 <= n < 2^40";
    p->Q = Q;
    p->first = first;
    p->n = n;
    return nullptr;
}
// out[i] = period[(phase + first + i) mod Q]; Mem: ld_tab(const uint8_t *period, int index)
template <class Mem> SK_HD void pn_chunk(const Mem &m, const PnPlan &p, const uint8_t *period, int64_t phase, uint8_t *out, int64_t c)
{
    int64_t e0;
    int a, b;
    if (!byte_chunk(out, p.n, c, &e0, &a, &b)) return;
    int at = (int)((uint64_t)(phase + p.first + e0 + a) % (uint64_t)p.Q);
    Bytes16 v = {{0, 0, 0, 0}};
SK_UNROLL
    for (int j = 0; j < 16; ++j) {
        if (j >= a && j < b) {
            put_byte(v, j, m.ld_tab(period, at) & 1u);
            at = at + 1 == p.Q ? 0 : at + 1;
        }
    }
    store_chunk(m, out, e0, a, b, v);
}

// ------------------------------------------------------------------------------------------------------------------ sigma and gain
// var = np.var of the row (M2 / n).  kSigmaAwgn: cpx_awgn's sigma = sqrt(ns var p / 2), g = 1, p = 10^(-es_n0 / 10);
// kSigmaAwgn2: cpx_awgn2's sigma = sqrt(var_w / 2), g = sqrt(1 / ns var_w / var p), p = 10^(es_n0 / 10): the reference's order
SK_HD void sigma_gain(int mode, double var, double ns, double p, double var_w, double *g, double *sigma)
{
    SK_NO_CONTRACT
    if (mode == kSigmaAwgn) {
        *sigma = sqrt_rn(ns * var * p / 2.0);
        *g = 1.0;
    } else {
        *sigma = sqrt_rn(var_w / 2.0);
        *g = sqrt_rn(1.0 / ns * var_w / var * p);
    }
}

}  // namespace chan
}  // namespace skdsp
