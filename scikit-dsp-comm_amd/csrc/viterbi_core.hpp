// viterbi_core.hpp -- the plan, the trellis and the per-state step of the register-exchange Viterbi decoder behind
// fec_conv.FECConv.viterbi_decoder (fec_conv.py:252-499 of the reference).  Plain C++ for host and device: viterbi.hip builds its
// kernels from it and tests/host/viterbi_emul.cpp walks the same functions lane by lane without a GPU.
//
// The code: R = 2 or 3 polynomials of K binary digits.  The encoder's K - 1 state bits read as a binary number with the NEWEST bit as the
// most significant one (the reference's state string), so state m is entered from p0 = 2 (m mod Ns/2) and p0 + 1 (Ns = 2^(K-1)) under the
// input bit m >> (K - 2).  The branch p -> m emits the word branch_word(p, u): bit R - 1 - j is the parity of polynomial j over the register
// [u, p].  The reference's rate-1/2 encoder feeds u into both outputs whatever the polynomials' first digits are; its rate-1/3 encoder
// honours them (fec_conv.py:517-553).  plan_make() folds that into the masks.
//
// The decoder (per received symbol, every state m at once):
//     d1 = bm(word(p0, u)) + metric[p0],  d2 = bm(word(p0 + 1, u)) + metric[p0 + 1]
//     d1 <= d2 keeps p0 (a tie keeps the even predecessor), else p0 + 1
//     history[m] = (history[kept] << 1) | u          -- the last Depth decided bits, newest in bit 0
// and the decided bit is bit Depth - 1 of the history of the FIRST state whose new metric is the minimum, from step Depth - 1 on.
// The history words hold 32 W >= Depth bits; the bits above Depth - 1 are older decisions nobody reads, so nothing is masked.
//
// Metrics.  hard: sum |x - b| over the symbol's values, x in {0, 1} (a value the stream ends before counts nothing).  soft: sum
// (int(x) - b top)^2, top = 2^quant_level - 1.  Both are integers, kept in int32 and NORMALISED: every step subtracts the step's minimum
// (which the output needs anyway).  Every decision -- d1 <= d2, the minimum's position -- depends on metric differences only and the
// reference's float64 sums are exact integers, so the bits are the reference's; a metric never exceeds (K - 1) bm_max after the
// subtraction (each state is reached from the minimum state of K - 1 steps earlier), K bm_max before it: with |int(x)| <= kSoftMaxAbs and
// quant_level <= kSoftMaxQuant that is 9 * 3 * 8190^2 = 1.81e9 < 2^31.  unquant: float64, (x - b)^2 summed in value order and then added
// to the predecessor's metric, one rounding per operation in the reference's order (dmul / dadd below never contract), not normalised.
#pragma once
#include <stdint.h>
#include <string.h>
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#ifndef SK_HD
#define SK_HD __host__ __device__ __forceinline__
#endif
#ifndef SK_UNROLL
#define SK_UNROLL _Pragma("unroll")
#endif
#else
#ifndef SK_HD
#define SK_HD inline
#endif
#ifndef SK_UNROLL
#define SK_UNROLL
#endif
#endif

namespace skdsp {
namespace vit {

constexpr int kMinK = 3, kMaxK = 9;       // the reference's whole polynomial table
constexpr int kMaxDepth = 128, kMaxWords = 4;
constexpr int kSoftMaxAbs = 4095, kSoftMaxQuant = 12;
constexpr int kWave = 64;
enum Metric { kHard = 0, kSoft = 1, kUnquant = 2 };
enum XType { kI8 = 0, kI16 = 1, kF64 = 2 };   // the received values as the kernel reads them: hard, soft (truncated), unquant
constexpr int kAbsent = -1;                // hard: a value behind the end of the stream

struct Plan {
    int K = 0, Ns = 0, R = 0, depth = 0;
    int words = 0;      // 32-bit words per history as instantiated: 2 (Depth <= 64) or 4
    int spl = 1;        // states per lane: 1 (Ns <= 64), 2, 4
    int streams = 1;    // independent streams sharing a wave in the rows form: 64 / Ns (Ns <= 64)
    int block = 0;      // symbols a stream loads at a time
    uint32_t gmask[3] = {0, 0, 0};
};

// lanes a stream occupies / loads of one symbol per lane that make a block
constexpr int lanes_of(int K) { return (1 << (K - 1)) < kWave ? (1 << (K - 1)) : kWave; }
constexpr int loads_of(int K) { return kWave / lanes_of(K) < 4 ? kWave / lanes_of(K) : 4; }

// 0, or the complaint (a static string)
inline const char *plan_make(const char *const *polys, int npoly, int depth, Plan *p)
{
    if (npoly != 2 && npoly != 3) return "Invalid rate. Use Rate 1/2 or 1/3 only";
    if (!polys || !polys[0]) return "null polynomial";
    const int K = (int)strlen(polys[0]);
    if (K < kMinK || K > kMaxK) return "the constraint length (digits per polynomial) must be 3 ... 9";
    if (depth < 1 || depth > kMaxDepth) return "Depth must be 1 ... 128";
    p->K = K;
    p->Ns = 1 << (K - 1);
    p->R = npoly;
    p->depth = depth;
    p->words = depth <= 64 ? 2 : 4;
    p->spl = p->Ns > kWave ? p->Ns / kWave : 1;
    p->streams = kWave / lanes_of(K);
    p->block = lanes_of(K) * loads_of(K);
    for (int j = 0; j < npoly; ++j) {
        if (!polys[j] || (int)strlen(polys[j]) != K) return "the polynomials must have the same number of digits";
        uint32_t m = 0;
        for (int i = 0; i < K; ++i) {
            if (polys[j][i] != '0' && polys[j][i] != '1') return "the polynomials must be strings of 0 and 1";
            m = (m << 1) | (uint32_t)(polys[j][i] - '0');
        }
        if (npoly == 2) m |= 1u << (K - 1);
        p->gmask[j] = m;
    }
    return nullptr;
}

// ---- trellis
SK_HD int pred0(int m, int Ns) { return 2 * (m & (Ns / 2 - 1)); }
SK_HD unsigned in_bit(int m, int K) { return (unsigned)m >> (K - 2); }
SK_HD unsigned branch_word(const uint32_t *gmask, int R, int K, int p, unsigned u)
{
    const uint32_t reg = (u << (K - 1)) | (uint32_t)p;
    unsigned w = 0;
    for (int j = 0; j < R; ++j) w = (w << 1) | ((unsigned)__builtin_popcount(reg & gmask[j]) & 1u);
    return w;
}

// ---- lanes.  Ns <= 64: lane = stream * Ns + state, one state per lane.  Ns > 64: lane l holds states l + 64 slot.
SK_HD int state_of(int lane, int slot, int Ns) { return Ns <= kWave ? lane % Ns : lane + kWave * slot; }
// where the even predecessor of this lane's states lives (the odd one: the next lane, same slot).  States slot = jj and jj + spl / 2 share it.
SK_HD int pred_lane(int lane, int Ns) { return Ns <= kWave ? lane - lane % Ns + pred0(lane % Ns, Ns) : (2 * lane) & (kWave - 1); }
SK_HD int pred_slot(int lane, int jj, int Ns) { return Ns <= kWave ? 0 : (lane >> 5) + 2 * jj; }

// ---- arithmetic: one rounding per operation on the device, like the host's (built with -ffp-contract=off)
#if defined(__HIP_DEVICE_COMPILE__)
SK_HD double dadd(double a, double b) { return __dadd_rn(a, b); }
SK_HD double dmul(double a, double b) { return __dmul_rn(a, b); }
#else
SK_HD double dadd(double a, double b) { return a + b; }
SK_HD double dmul(double a, double b) { return a * b; }
#endif
SK_HD int madd(int a, int b) { return a + b; }
SK_HD double madd(double a, double b) { return dadd(a, b); }

// the distance of one received value to code bit b
SK_HD int dist_hard(int v, int b) { return v < 0 ? 0 : (v ^ b); }
SK_HD int dist_soft(int v, int b, int top) { const int d = v - b * top; return d * d; }
SK_HD double dist_unquant(double v, int b) { const double d = v - (double)b; return dmul(d, d); }

// a symbol's R values against both code bits: d[k][b]
template <int METRIC> struct Dist;
template <> struct Dist<kHard> {
    typedef int MT;
    SK_HD static void both(const int *v, int R, int, int (*d)[2])
    {
        for (int k = 0; k < R; ++k) { d[k][0] = dist_hard(v[k], 0); d[k][1] = dist_hard(v[k], 1); }
    }
};
template <> struct Dist<kSoft> {
    typedef int MT;
    SK_HD static void both(const int *v, int R, int top, int (*d)[2])
    {
        for (int k = 0; k < R; ++k) { d[k][0] = dist_soft(v[k], 0, top); d[k][1] = dist_soft(v[k], 1, top); }
    }
};
template <> struct Dist<kUnquant> {
    typedef double MT;
    SK_HD static void both(const double *v, int R, int, double (*d)[2])
    {
        for (int k = 0; k < R; ++k) { d[k][0] = dist_unquant(v[k], 0); d[k][1] = dist_unquant(v[k], 1); }
    }
};

// the branch metric of code word `word` (first value = most significant bit), summed in value order
template <typename MT> SK_HD MT branch_metric(const MT (*d)[2], int R, unsigned word)
{
    MT s = ((word >> (R - 1)) & 1u) ? d[0][1] : d[0][0];
    s = madd(s, ((word >> (R - 2)) & 1u) ? d[1][1] : d[1][0]);
    if (R == 3) s = madd(s, (word & 1u) ? d[2][1] : d[2][0]);
    return s;
}

// add-compare-select and history update of ONE state: predecessor metrics pm0 / pm1 (even / odd), their branch metrics and histories
template <typename MT, int W>
SK_HD void acs(MT pm0, MT pm1, MT bm0, MT bm1, const uint32_t *h0, const uint32_t *h1, unsigned u, MT *m, uint32_t *h)
{
    const MT d1 = madd(bm0, pm0), d2 = madd(bm1, pm1);
    const bool keep0 = d1 <= d2;
    *m = keep0 ? d1 : d2;
    uint32_t carry = u;
    SK_UNROLL
    for (int w = 0; w < W; ++w) {
        const uint32_t src = keep0 ? h0[w] : h1[w];
        h[w] = (src << 1) | carry;
        carry = src >> 31;
    }
}
SK_HD unsigned oldest_bit(const uint32_t *h, int depth) { return (h[(depth - 1) >> 5] >> ((depth - 1) & 31)) & 1u; }

// output length: symbols = ceil(values / R) (hard takes a short last symbol), one decided bit per symbol from symbol Depth - 1 on
inline int64_t symbols_of(const Plan &p, int64_t nval) { return (nval + p.R - 1) / p.R; }
inline int64_t out_len(const Plan &p, int64_t nval)
{
    const int64_t n = symbols_of(p, nval) - (p.depth - 1);
    return n > 0 ? n : 0;
}
// the decoder state a handle carries from call to call: Ns metrics in 8-byte cells (int32 in the low half, or float64), then Ns histories
// of kMaxWords words
inline size_t state_bytes(const Plan &p) { return (size_t)p.Ns * (8 + 4 * kMaxWords); }

}  // namespace vit
}  // namespace skdsp
