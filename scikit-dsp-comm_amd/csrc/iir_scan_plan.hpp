// iir_scan_plan.hpp -- the plan of the cascade scans (iir_scan.hip, iir_fused.hip) without a device: the one-step transition matrix of a
// cascade, the tables of a chunk length T, the geometry of a call, and the rules that admit the matrix-pipe K1, the interleaved two-pass
// kernels and the single pass.  Standard headers only: tests/host/iir_scan_plan_emul.cpp runs it on the host; iir_api.hip uploads what it
// makes, and every launch checks its own rule from here.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace skdsp {

constexpr int kIirThreads = 256;
constexpr int kPiece = 32;          // samples per thread per staged piece
constexpr int kMmPiece = 128;       // samples of every chunk the matrix-pipe K1 stages at a time
constexpr int kMaxPairs = 12288;    // K2 capacity: workgroups x state dimension (one 96 KiB LDS image)
constexpr int kMaxW = 512;          // workgroups (of 256 chunks) per vector (1024 measured slower: more scan, same occupancy)
constexpr int kPowers = 19;         // M^(2^l), l = 0..18

// one cascade step on the host (long double) -- used to build the transition matrix.  coef: per section b[0..order], a[1..order]
inline void host_step(const double *coef, int nsec, int ORD, std::vector<long double> &z, long double x)
{
    for (int s = 0; s < nsec; ++s) {
        const double *c = coef + (size_t)s * (2 * ORD + 1);
        const long double xn = x;
        const long double yv = (long double)c[0] * xn + z[s * ORD];
        for (int k = 1; k < ORD; ++k) z[s * ORD + k - 1] = (long double)c[k] * xn - (long double)c[ORD + k] * yv + z[s * ORD + k];
        z[s * ORD + ORD - 1] = (long double)c[ORD] * xn - (long double)c[2 * ORD] * yv;
        x = yv;
    }
}

inline void matmul_ld(const std::vector<long double> &A, const std::vector<long double> &B, std::vector<long double> &C, int D)
{
    std::vector<long double> R((size_t)D * D, 0.0L);
    for (int i = 0; i < D; ++i)
        for (int k = 0; k < D; ++k) {
            const long double a = A[(size_t)i * D + k];
            if (a == 0.0L) continue;
            for (int j = 0; j < D; ++j) R[(size_t)i * D + j] += a * B[(size_t)k * D + j];
        }
    C.swap(R);
}

// one-step transition, D x D row-major: column i = state after a zero-input step from e_i
inline std::vector<double> scan_A_host(const double *coef, int nsec, int order)
{
    const int D = nsec * order;
    std::vector<double> A((size_t)D * D, 0.0);
    for (int i = 0; i < D; ++i) {
        std::vector<long double> z(D, 0.0L);
        z[i] = 1.0L;
        host_step(coef, nsec, order, z, 0.0L);
        for (int r = 0; r < D; ++r) A[(size_t)r * D + i] = (double)z[r];
    }
    return A;
}

// the tables of one chunk length T (M = A^T is the transition over a chunk)
struct ScanTables {
    std::vector<double> pw;    // kPowers matrices M^(2^l), each D x D row-major
    std::vector<double> pwa;   // M^(2^l), l = 0..7, zero-padded to 16 x 16, as MFMA A operands [l][k / 4][64] (D <= 16, else zeros)
    std::vector<double> lb;    // look-back matrices (M^256)^k, k = 1..7, at [k - 1]
    std::vector<double> lbk;   // M^k, k = 0..31, transposed so that lane k reads entry (i,j) at [(i*D+j)*32 + k]
    std::vector<double> gt;    // G = [A^(T-1-k) b]_k in MFMA A-operand order (empty where gt_T < 0)
    int64_t gt_T = -1;         // T where the G table was made, else -1
    int n_lb = 0;              // terms of the in-kernel carry look-back (0 = use the K2 scan)
    int n_lv = kPowers;        // first l with max|M^(2^l)| < negl (chunk-level scan depth that matters)
};

// A transition power counts as vanished when its largest entry is below `negl`: 1e-30 for float64 signals (nothing a
// float64 recurrence could resolve), 1e-18 for float32 signals (the dropped term is under a tenth of an ulp of the
// float64 STATE it would be added to, and eleven orders below the float32 rounding of the output) -- for the config-4
// cascade (pole radius 0.99465) that is 60 chunks of 128 samples instead of 101: one scan level less.
inline long double scan_negl(bool dbl) { return dbl ? 1e-30L : 1e-18L; }

inline ScanTables scan_tables(const double *coef, int nsec, int order, const std::vector<double> &A_host, int64_t T, bool dbl)
{
    ScanTables t;
    const int D = nsec * order;
    std::vector<long double> base((size_t)D * D), M((size_t)D * D, 0.0L);
    for (size_t i = 0; i < base.size(); ++i) base[i] = A_host[i];
    for (int i = 0; i < D; ++i) M[(size_t)i * D + i] = 1.0L;
    // M = A^T by binary exponentiation
    int64_t e = T;
    std::vector<long double> sq = base;
    while (e) {
        if (e & 1) matmul_ld(M, sq, M, D);
        e >>= 1;
        if (e) matmul_ld(sq, sq, sq, D);
    }
    {
        std::vector<long double> Pk((size_t)D * D, 0.0L);
        for (int i = 0; i < D; ++i) Pk[(size_t)i * D + i] = 1.0L;
        t.lbk.resize((size_t)32 * D * D);
        for (int k = 0; k < 32; ++k) {
            for (size_t i = 0; i < (size_t)D * D; ++i) t.lbk[i * 32 + k] = std::isfinite((double)Pk[i]) ? (double)Pk[i] : 0.0;
            matmul_ld(Pk, M, Pk, D);
        }
    }
    if (D <= 32 && (T % kMmPiece == 0 || T == 64 || T == 32)) {
        // G[:, k] = A^(T-1-k) b, b = the state one sample x = 1 leaves behind; stored as the MFMA A operand
        // of step s = k / 4: lane l holds row l & 15, column 4 s + (l >> 4)
        std::vector<long double> g(D, 0.0L);
        host_step(coef, nsec, order, g, 1.0L);
        const int NT = D > 16 ? 2 : 1;
        t.gt.assign((size_t)NT * T * 16, 0.0);
        for (int64_t k = T - 1; k >= 0; --k) {
            for (int d = 0; d < D; ++d) {
                const long double v = g[d];
                t.gt[(size_t)(d / 16) * T * 16 + (size_t)(k / 4) * 64 + (size_t)(k % 4) * 16 + (d % 16)] = std::isfinite((double)v) ? (double)v : 0.0;
            }
            host_step(coef, nsec, order, g, 0.0L);  // g <- A g
        }
        t.gt_T = T;
    }
    const long double negl = scan_negl(dbl);
    t.pw.resize((size_t)kPowers * D * D);
    for (int l = 0; l < kPowers; ++l) {
        long double mx = 0.0L;
        for (auto v : M) mx = fabsl(v) > mx ? fabsl(v) : mx;
        if (std::isfinite((double)mx) && mx < negl && l < t.n_lv) t.n_lv = l;
        for (size_t i = 0; i < (size_t)D * D; ++i) {
            long double v = M[i];
            if (!std::isfinite((double)v)) v = 0.0L;  // unstable filter overflow: the reference overflows too
            t.pw[(size_t)l * D * D + i] = (double)v;
        }
        if (l + 1 < kPowers) matmul_ld(M, M, M, D);
    }
    // carry look-back: (M^256)^k until every entry is below negl (its contribution is then far
    // under one ulp of anything the float64 recurrence itself could resolve)
    {
        std::vector<long double> Mw((size_t)D * D), Pk;
        for (size_t i = 0; i < (size_t)D * D; ++i) Mw[i] = t.pw[(size_t)8 * D * D + i];
        Pk = Mw;
        t.lb.assign((size_t)8 * D * D, 0.0);
        for (int k = 1; k <= 8; ++k) {  // Pk = Mw^k
            long double mx = 0.0L;
            for (auto v : Pk) mx = fabsl(v) > mx ? fabsl(v) : mx;
            if (!(mx >= negl)) { t.n_lb = k; break; }  // terms k.. are negligible: keep k terms (0..k-1)
            if (k == 8) break;
            for (size_t i = 0; i < (size_t)D * D; ++i) t.lb[(size_t)(k - 1) * D * D + i] = (double)Pk[i];
            matmul_ld(Pk, Mw, Pk, D);
        }
    }
    t.pwa.assign((size_t)8 * 4 * 64, 0.0);
    if (D <= 16) {  // the same powers as A operands of v_mfma_f64_16x16x4: step r of level l, lane t: M_l[t & 15][4 r + (t >> 4)]
        for (int l = 0; l < 8; ++l)
            for (int r = 0; r < 4; ++r)
                for (int tt = 0; tt < 64; ++tt) {
                    const int row = tt & 15, col = 4 * r + (tt >> 4);
                    if (row < D && col < D) t.pwa[((size_t)l * 4 + r) * 64 + tt] = t.pw[(size_t)l * D * D + (size_t)row * D + col];
                }
    }
    return t;
}

// ---- the geometry of a two-pass call: J chunks of T samples, W workgroups of 256 chunks -------------------------------------
struct ScanGeom { int maxW; int64_t T, J; int W; };
inline ScanGeom scan_geometry(int64_t n, int D)
{
    ScanGeom g;
    g.maxW = kMaxPairs / D;
    if (g.maxW > kMaxW) g.maxW = kMaxW;
    const int64_t maxChunks = (int64_t)g.maxW * kIirThreads;
    int64_t T = (n + maxChunks - 1) / maxChunks;
    T = ((T + kPiece - 1) / kPiece) * kPiece;
    if (T < kPiece) T = kPiece;
    if (T >= kMmPiece) T = ((T + kMmPiece - 1) / kMmPiece) * kMmPiece;  // whole 128-sample pieces for the matrix-pipe K1
    g.T = T;
    g.J = (n + T - 1) / T;
    g.W = (int)((g.J + kIirThreads - 1) / kIirThreads);
    return g;
}
// the decimating store: samples between a thread's staged segments (the interleaved complex kernel stages 8 segments per row piece), div / mod dec
inline int64_t scan_dec_step(bool interleaved, bool dbl, int64_t T) { return (interleaved ? kIirThreads / 8 : kIirThreads / (kPiece / (16 / (dbl ? 8 : 4)))) * T; }
inline int scan_dec_dq(bool interleaved, bool dbl, int64_t T, int dec) { return (int)(scan_dec_step(interleaved, dbl, T) / dec); }
inline int scan_dec_dr(bool interleaved, bool dbl, int64_t T, int dec) { return (int)(scan_dec_step(interleaved, dbl, T) % dec); }

// ---- which kernels a call takes ----------------------------------------------------------------------------------------------
// what the rules read of the tables of a chunk length
struct ScanFacts { int n_lv, n_lb; int64_t gt_T; };
// aggregate-free mode: matrix-pipe K1, carries from the chunk states themselves, unchanged K3
inline bool scan_fast(const ScanFacts &f, int D, int order, int64_t T, int iir_no_mfma)
{
    return f.n_lv <= 5 && D <= 32 && order == 2 && T % kMmPiece == 0 && f.gt_T == T && !iir_no_mfma;
}
// the interleaved complex two-pass kernels (iir_k1c / iir_k3c): aggregate-free mode only
inline bool scan_interleaved_applies(bool fast, int64_t T) { return fast && T % 64 == 0; }

// K1 of a two-pass call: the per-thread cascade (and workgroup aggregates), or in aggregate-free mode v = G x on the matrix pipe -- with G in
// registers (persistent workgroups) where D <= 16 and the chunk is 1, 2 or 4 pieces, else staged per piece; interleaved signals: staged
enum ScanK1 { kK1Chunk, kK1Regs, kK1Mfma };
inline int scan_k1(bool fast, bool interleaved, int D, int64_t T)
{
    if (!fast) return kK1Chunk;
    const int64_t np = T / kMmPiece;
    return !interleaved && D <= 16 && (np == 1 || np == 2 || np == 4) && T == np * kMmPiece ? kK1Regs : kK1Mfma;
}
// the form of a two-pass launch, decided before it
struct ScanForm { bool fast; bool unit_tail; int k1; };

// Single-pass scan (iir_fused.hip; one launch, x read once): <= 8 biquads whose transition over one 256-chunk segment vanishes (n_lb == 1
// for the segment's chunk length), enough segments to fill the chip.
// chunk length: 128 float32 / 64 float64 samples (real), 64 complex64 / 32 complex128 samples (interleaved)
inline int64_t fused_chunk(bool dbl, bool interleaved) { return (dbl ? 64 : 128) / (interleaved ? 2 : 1); }
// fstate: the cached applicability (0 untested, 1 applicable, -1 not)
inline bool fused_wanted(int order, int D, int iir_two_pass, int fstate, int dec, int nbatch, bool interleaved, bool zf, int64_t n, bool dbl, int num_cus)
{
    return order == 2 && D <= 16 && iir_two_pass <= 0 && fstate >= 0 && (dec <= 1 || ((nbatch == 1 || interleaved) && !zf)) &&
           n >= fused_chunk(dbl, interleaved) * kIirThreads * (int64_t)num_cus;
}
inline bool fused_applies(const ScanFacts &at_Tf, int64_t Tf) { return at_Tf.n_lb == 1 && at_Tf.gt_T == Tf; }
// The policy, per call.  Real signals: the single pass wins or ties everywhere it applies (tools/ab_iir.py, 2^26, same box): low-pass designs
// 0.11-0.13 vs 0.15 ms, float64 0.19-0.28 vs 0.36-0.42 ms; the 8-biquad elliptic band-pass of BASELINE config 4
// (6 scan levels of a 16 x 16 transition per 128-sample chunk) 0.175 vs 0.184 ms since its scan runs on the
// matrix pipe (iir_fused.hip: 0.197 ms with the per-thread VALU scan) -- and it moves 8 instead of 12 bytes per sample.
// interleaved complex64 (two scans per 64-sample chunk): 0.22-0.29 vs 0.42-0.45 ms for low-pass designs (<= 4
// levels), 0.56 vs 0.46 ms for the config-4 cascade (7 levels): those stay two-pass unless iir_two_pass = -1
inline bool fused_policy(bool interleaved, bool dbl, int fnlv, int iir_two_pass) { return !(interleaved && !dbl && fnlv >= 6 && iir_two_pass >= 0); }

}  // namespace skdsp
