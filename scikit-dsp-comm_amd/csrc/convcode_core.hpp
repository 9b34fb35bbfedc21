// convcode_core.hpp -- the plans, the staging and the per-item functions of the FEC chain kernels around the Viterbi decoder:
// fec_conv.FECConv.conv_encoder / puncture / depuncture (fec_conv.py:501-712 of the reference) and the count behind
// digitalcom.bit_errors (digitalcom.py:353-415).  Plain C++ for host and device: convcode.hip builds its kernels from it and
// tests/host/convcode_emul.cpp walks the same functions thread by thread without a GPU.
//
// Encoder.  A GF(2) FIR: output bit j of polynomial p at input t is the parity of the polynomial's mask over the register [u[t], u[t-1], ...
// u[t-K+1]] (the masks and the rate-1/2 rule are viterbi_core.hpp's plan_make: the decoder's trellis and this encoder cannot disagree).
// u[-1-m] is digit m of the row's initial state string (newest first).  A work item is (row, run of kEncWg bits); a lane takes kEncRun of
// them.  The item's window -- its bits and the K - 1 bytes in front of them where the row has them -- is staged into an LDS image by
// blockcode_core.hpp's stage_in (aligned 16-byte chunks, heads and tails by byte), the lane packs its bits and the K - 1 before them into
// one word w (bit K - 1 + j = u[lane's first bit + j]), polynomial p's 16 outputs are the XOR of (w >> s) over the set bits s of its mask,
// the R words are interleaved into the output image, and stage_out stores the item's R * bits bytes.  The final state is the last K - 1
// inputs, newest first: bits of the w of the lane that holds the row's last bit.
//
// Puncture / depuncture.  Both are one periodic gather: output element o = q P_out + r reads input element q P_in + tab[r], or takes the
// erase value where tab[r] = kErase.  The table of one period is built on the host from the two pattern masks (gather_plan_make).
//
// Count.  Row r: the number of i < n whose tx and rx bytes differ in bit 0 (invert: agree).  A work item is (row, kCntWg bytes); both
// streams are staged at their own alignment, the item's sum is added to the row's int64 with an integer atomic: the total does not depend
// on the order.
#pragma once
#include "viterbi_core.hpp"
#include "blockcode_core.hpp"

namespace skdsp {
namespace cvc {

// ------------------------------------------------------------------------------------------------------------------ encoder
constexpr int kThreads = 256;
constexpr int kEncRun = 16;                    // bits per lane
constexpr int kEncWg = kThreads * kEncRun;     // bits per work item
constexpr int kHist = 8;                       // kMaxK - 1: the most bytes staged in front of an item's bits
// input image: the window at its global alignment (lead < 16); output image: R * kEncWg bytes at theirs
constexpr int kEncInBytes = blk::image_bytes(kEncWg + kHist);
constexpr int kEncOutBytes = blk::image_bytes(3 * kEncWg);

struct EncPlan {
    int K = 0, R = 0;
    uint32_t gmask[3] = {0, 0, 0};
};

inline const char *enc_plan_make(const char *const *polys, int npoly, EncPlan *p)
{
    vit::Plan v;
    const char *why = vit::plan_make(polys, npoly, 1, &v);
    if (why) return why;
    p->K = v.K;
    p->R = v.R;
    for (int j = 0; j < 3; ++j) p->gmask[j] = v.gmask[j];
    return nullptr;
}

inline int64_t enc_items_per_row(int64_t n) { return (n + kEncWg - 1) / kEncWg; }
// item `it` of a row of n bits: its first bit, its bits, the bytes staged in front of them
SK_HD int64_t enc_first(int64_t it) { return it * kEncWg; }
SK_HD int enc_len(int64_t n, int64_t it) { const int64_t left = n - it * kEncWg; return left < kEncWg ? (int)left : kEncWg; }
SK_HD int enc_hist(const EncPlan &p, int64_t it) { return it > 0 ? p.K - 1 : 0; }

// The lane's word.  img: the input image (window byte i at img[lead + i]); h: bytes of history in the window; len: the item's bits;
// i0: the lane's first bit within the item; state: the row's initial state as a number (digit 0 = bit K - 2).  Bit K - 1 + j of the word
// is bit i0 + j of the item (j < 0: the bits before it), 0 beyond the item's end.
SK_HD uint32_t enc_lane_word(const EncPlan &p, const uint8_t *img, int lead, int h, int len, int i0, uint32_t state)
{
    uint32_t w = 0;
    const int K1 = p.K - 1;
    for (int j = -K1; j < kEncRun; ++j) {
        const int i = i0 + j;
        if (i >= -h && i < len) w |= (uint32_t)(img[lead + h + i] & 1u) << (K1 + j);
    }
    if (h == 0 && i0 == 0) w |= state;   // the row's first lane: u[-1-m] = state digit m = bit K - 2 - m
    return w;
}
// the 16 outputs of polynomial j: the XOR of the shifts its mask selects
SK_HD uint32_t enc_poly_word(const EncPlan &p, uint32_t w, int j)
{
    uint32_t o = 0;
    for (int s = 0; s < vit::kMaxK; ++s)
        if ((p.gmask[j] >> s) & 1u) o ^= w >> s;
    return o & ((1u << kEncRun) - 1u);
}
// the lane's R * cnt output bytes, [p0 p1 (p2)] per bit, at out[0 ...)
SK_HD void enc_put(const EncPlan &p, uint32_t w, int cnt, uint8_t *out)
{
    const uint32_t o0 = enc_poly_word(p, w, 0), o1 = enc_poly_word(p, w, 1), o2 = p.R == 3 ? enc_poly_word(p, w, 2) : 0u;
    for (int j = 0; j < cnt; ++j) {
        out[p.R * j] = (uint8_t)((o0 >> j) & 1u);
        out[p.R * j + 1] = (uint8_t)((o1 >> j) & 1u);
        if (p.R == 3) out[3 * j + 2] = (uint8_t)((o2 >> j) & 1u);
    }
}
// the state behind the lane's bit jl (its last one): the K - 1 newest inputs, newest = bit K - 2
SK_HD uint32_t enc_state_after(const EncPlan &p, uint32_t w, int jl) { return (w >> (jl + 1)) & ((1u << (p.K - 1)) - 1u); }

// ------------------------------------------------------------------------------------------------------------------ puncture / depuncture
constexpr int kMaxPattern = 64;
constexpr int kErase = 255;
constexpr int kGatherPerThread = 4;

struct GatherPlan {
    int p_in = 0, p_out = 0;             // elements per period on each side
    uint8_t tab[2 * kMaxPattern] = {};   // the input offset of output r of a period, or kErase
};

inline int ones_of(uint64_t m) { return __builtin_popcountll(m); }
// digit k of a pattern string is bit k of its mask.  0, or the complaint
inline const char *pattern_check(uint64_t mask1, uint64_t mask2, int L_pp)
{
    if (L_pp < 1 || L_pp > kMaxPattern) return "the puncture pattern must have 1 ... 64 digits";
    if (L_pp < 64 && ((mask1 >> L_pp) || (mask2 >> L_pp))) return "a pattern mask has digits beyond the pattern's length";
    if (ones_of(mask1) != ones_of(mask2)) return "the two patterns must keep the same number of bits";
    if (ones_of(mask1) == 0) return "the puncture pattern keeps no bit";
    return nullptr;
}
// the one place the output lengths come from: n elements of a row -> elements of the punctured / depunctured row
inline int64_t puncture_out_len(int64_t n, uint64_t mask1, int L_pp) { return (n / 2 / L_pp) * 2 * ones_of(mask1); }
inline int64_t depuncture_out_len(int64_t n, uint64_t mask1, int L_pp) { return (n / 2 / ones_of(mask1)) * 2 * L_pp; }

inline void gather_plan_make(uint64_t mask1, uint64_t mask2, int L_pp, bool depuncture, GatherPlan *g)
{
    const int L1 = ones_of(mask1);
    const uint64_t mask[2] = {mask1, mask2};
    g->p_in = depuncture ? 2 * L1 : 2 * L_pp;
    g->p_out = depuncture ? 2 * L_pp : 2 * L1;
    for (int s = 0; s < 2; ++s) {
        int rank = 0;
        for (int k = 0; k < L_pp; ++k) {
            const bool kept = (mask[s] >> k) & 1u;
            if (depuncture) g->tab[2 * k + s] = kept ? (uint8_t)(2 * rank + s) : (uint8_t)kErase;
            else if (kept) g->tab[2 * rank + s] = (uint8_t)(2 * k + s);
            rank += kept;
        }
    }
}
inline int64_t gather_items_per_row(int64_t n_out) { return (n_out + kThreads * kGatherPerThread - 1) / (kThreads * kGatherPerThread); }
// Thread t of item `it` of a row: output elements it * 1024 + t + 256 u, u < kGatherPerThread.  One division; from element to element the
// period q and the place r in it advance by 256 / P_out and 256 mod P_out.  Mem does the element accesses (ld / st).
template <typename T, class Mem>
SK_HD void gather_thread(const Mem &m, const uint8_t *tab, int p_in, int p_out, const T *x, T *y, int64_t n_out, T erase, uint32_t it, int t)
{
    const uint32_t P = (uint32_t)p_out, dq = kThreads / P, dr = kThreads % P;
    int64_t o = (int64_t)it * (kThreads * kGatherPerThread) + t;
    int64_t q = o / P;
    uint32_t r = (uint32_t)(o - q * P);
    SK_UNROLL
    for (int u = 0; u < kGatherPerThread; ++u) {
        if (o < n_out) {
            const int s = tab[r];
            m.st(y + o, s == kErase ? erase : m.ld(x + q * p_in + s));
        }
        o += kThreads;
        q += dq;
        r += dr;
        if (r >= P) {
            r -= P;
            ++q;
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------ count
constexpr int kCntWg = kThreads * 16;          // bytes of a row per work item, 16 per lane
constexpr int kCntImgBytes = blk::image_bytes(kCntWg);
inline int64_t cnt_items_per_row(int64_t n) { return (n + kCntWg - 1) / kCntWg; }
// the lane's share: bytes [i0, i0 + 16) of the item's len, from the two images at their own leads
SK_HD int cnt_lane(const uint8_t *img_t, int lead_t, const uint8_t *img_r, int lead_r, int len, int i0, int invert)
{
    int c = 0;
    for (int j = 0; j < 16; ++j) {
        const int i = i0 + j;
        if (i < len) c += (int)(((img_t[lead_t + i] ^ img_r[lead_r + i]) & 1u) ^ (unsigned)invert);
    }
    return c;
}

}  // namespace cvc
}  // namespace skdsp
