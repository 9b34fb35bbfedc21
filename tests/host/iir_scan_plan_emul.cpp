// Host run of csrc/iir_scan_plan.hpp (standard headers only): the plan of the cascade scans on inputs whose tables are known in closed form,
// the geometry of a call on both sides of each rounding rule, and every launch rule on both sides of each of its conditions.
//   g++ -O1 -std=c++17 -I scikit-dsp-comm_amd/csrc tests/host/iir_scan_plan_emul.cpp && ./a.out
#include <cmath>
#include <cstdio>
#include <vector>
#include "iir_scan_plan.hpp"

using namespace skdsp;

static int g_fail = 0;
#define EXPECT(c) do { if (!(c)) { ++g_fail; printf("FAIL %s:%d  %s\n", __FILE__, __LINE__, #c); } } while (0)

static double p2(long k) { return (double)std::ldexp(1.0L, (int)-k); }   // 2^-k as the tables hold it (0 below the double range)

// one biquad y[n] = x[n] + 0.5 y[n-1]: A = [[1/2, 1], [0, 0]], so A^k = [[2^-k, 2^-(k-1)], [0, 0]] exactly
static void half_pole(int T)
{
    const double coef[5] = {1.0, 0.0, 0.0, -0.5, 0.0};
    const std::vector<double> A = scan_A_host(coef, 1, 2);
    EXPECT(A[0] == 0.5 && A[1] == 1.0 && A[2] == 0.0 && A[3] == 0.0);
    for (int dbl = 0; dbl < 2; ++dbl) {
        const ScanTables t = scan_tables(coef, 1, 2, A, T, dbl != 0);
        EXPECT(t.pw.size() == (size_t)kPowers * 4 && t.lb.size() == 32u && t.lbk.size() == 128u && t.pwa.size() == 2048u);
        for (int l = 0; l < kPowers; ++l) {   // pw[l] = M^(2^l) = A^(T 2^l)
            const long k = (long)T << l;
            EXPECT(t.pw[4 * l] == p2(k) && t.pw[4 * l + 1] == p2(k - 1) && t.pw[4 * l + 2] == 0.0 && t.pw[4 * l + 3] == 0.0);
        }
        // the largest entry of level l is 2^-(T 2^l - 1): T = 32: 4.7e-10, 1.1e-19, 5.9e-39; T = 128: 5.9e-39 at once
        EXPECT(t.n_lv == (T == 32 ? (dbl ? 2 : 1) : 0));
        EXPECT(t.n_lb == 1);   // M^256 is below the double range: the look-back is the neighbour alone
        for (double v : t.lb) EXPECT(v == 0.0);
        for (int k = 0; k < 32; ++k) {   // lbk: entry (i, j) of M^k at [(i D + j) 32 + k]
            EXPECT(t.lbk[0 * 32 + k] == (k ? p2((long)T * k) : 1.0) && t.lbk[1 * 32 + k] == (k ? p2((long)T * k - 1) : 0.0));
            EXPECT(t.lbk[2 * 32 + k] == 0.0 && t.lbk[3 * 32 + k] == (k ? 0.0 : 1.0));
        }
        // G[:, k] = A^(T-1-k) b with b = (1/2, 0): state d of sample k at [(d / 16) 16 T + (k / 4) 64 + (k % 4) 16 + d % 16]
        EXPECT(t.gt_T == T && t.gt.size() == (size_t)16 * T);
        for (int k = 0; k < T; ++k)
            for (int d = 0; d < 16; ++d) EXPECT(t.gt[(size_t)(k / 4) * 64 + (k % 4) * 16 + d] == (d == 0 ? p2(T - k) : 0.0));
        // pwa: step r of level l, lane t holds M_l[t & 15][4 r + (t >> 4)]
        for (int l = 0; l < 8; ++l)
            for (int r = 0; r < 4; ++r)
                for (int lane = 0; lane < 64; ++lane) {
                    const int row = lane & 15, col = 4 * r + (lane >> 4);
                    EXPECT(t.pwa[((size_t)l * 4 + r) * 64 + lane] == (row < 2 && col < 2 ? t.pw[4 * l + 2 * row + col] : 0.0));
                }
    }
}

// a pole at r = 1 - 2^-10: (M^256)^k for 32-sample chunks is r^(8192 k) ~ e^(-8 k): 4e-18 at k = 5, 1e-21 at k = 6, 1e-28 at k = 8 --
// float32 signals (1e-18) keep 6 terms, float64 signals (1e-30) scan the aggregates
static void slow_pole()
{
    const double r = 1.0 - std::ldexp(1.0, -10);
    const double coef[5] = {1.0, 0.0, 0.0, -r, 0.0};
    const std::vector<double> A = scan_A_host(coef, 1, 2);
    for (int dbl = 0; dbl < 2; ++dbl) {
        const ScanTables t = scan_tables(coef, 1, 2, A, 32, dbl != 0);
        const double negl = dbl ? 1e-30 : 1e-18;
        int want = 0;
        for (int k = 1; k <= 8 && !want; ++k)
            if (std::pow(r, 8192.0 * k - 1.0) < negl) want = k;
        EXPECT(want == (dbl ? 0 : 6) && t.n_lb == want);
        for (int k = 1; k < (want ? want : 8); ++k) EXPECT(std::fabs(t.lb[(size_t)(k - 1) * 4] / std::pow(r, 8192.0 * k) - 1.0) < 1e-9);
        // scan levels: r^(32 2^l - 1) < negl first at l = 11 (e^-64) for float32, l = 12 (e^-128) for float64
        EXPECT(t.n_lv == (dbl ? 12 : 11));
    }
}

// three sections: section s never sees the state of a later section, so row i of every power stops at the end of its own 2-wide block
static void block_triangular()
{
    const double coef[15] = {0.2, 0.1, 0.2, -1.2, 0.8, 1.0, -1.0, 0.5, 0.3, 0.4, 0.7, 0.2, 0.7, -0.9, 0.6};
    const int D = 6;
    const std::vector<double> A = scan_A_host(coef, 3, 2);
    for (int T : {32, 64, 96, 128, 256}) {
        const ScanTables t = scan_tables(coef, 3, 2, A, T, true);
        bool lower_used = false;
        for (int l = 0; l < kPowers; ++l)
            for (int i = 0; i < D; ++i)
                for (int j = 0; j < D; ++j) {
                    if (j >= (i / 2 + 1) * 2) EXPECT(t.pw[((size_t)l * D + i) * D + j] == 0.0);
                    else if (l == 0 && i >= 4 && j < 2 && t.pw[((size_t)l * D + i) * D + j] != 0.0) lower_used = true;
                }
        EXPECT(lower_used);   // (row-major M, not its transpose)
        EXPECT((t.gt_T == T) == (T != 96) && t.gt.empty() == (T == 96));   // G only where a matrix-pipe K1 exists: whole 128-sample pieces, 64, 32
    }
}

static void geometry()
{
    const int64_t chunks = (int64_t)kMaxW * kIirThreads;
    ScanGeom g = scan_geometry(1000, 2);
    EXPECT(g.maxW == kMaxW && g.T == 32 && g.J == 32 && g.W == 1);          // 12288 / 2 workgroups would fit K2: capped by kMaxW
    g = scan_geometry(1000, 48);
    EXPECT(g.maxW == kMaxPairs / 48 && g.maxW < kMaxW);                       // ... by K2's capacity
    g = scan_geometry(32 * chunks, 16);
    EXPECT(g.T == 32 && g.J == chunks && g.W == kMaxW);
    g = scan_geometry(32 * chunks + 1, 16);
    EXPECT(g.T == 64 && g.W == 257);                                         // whole 32-sample pieces
    g = scan_geometry(96 * chunks, 16);
    EXPECT(g.T == 96);                                                       // below 128: any multiple of 32
    g = scan_geometry(96 * chunks + 1, 16);
    EXPECT(g.T == 128 && g.J == (96 * chunks + 1 + 127) / 128);
    g = scan_geometry(128 * chunks + 1, 16);
    EXPECT(g.T == 256);                                                      // from 128 on: whole 128-sample pieces (160 is not one)
    g = scan_geometry(1, 2);
    EXPECT(g.T == 32 && g.J == 1 && g.W == 1);
    // samples between a thread's staged segments: 8 float32 / 16 float64 segments per 32-sample piece, 8 per interleaved row piece
    EXPECT(scan_dec_step(false, false, 128) == 32 * 128 && scan_dec_step(false, true, 64) == 16 * 64 && scan_dec_step(true, false, 64) == 32 * 64 &&
           scan_dec_step(true, true, 32) == 32 * 32);
    EXPECT(scan_dec_dq(false, false, 128, 3) == 4096 / 3 && scan_dec_dr(false, false, 128, 3) == 4096 % 3);
}

static void rules()
{
    const ScanFacts ok{5, 1, 128};
    EXPECT(scan_fast(ok, 16, 2, 128, 0));
    EXPECT(!scan_fast(ScanFacts{6, 1, 128}, 16, 2, 128, 0));   // six scan levels
    EXPECT(scan_fast(ok, 32, 2, 128, 0) && !scan_fast(ok, 34, 2, 128, 0));
    EXPECT(!scan_fast(ok, 16, 4, 128, 0));                     // biquads only
    EXPECT(!scan_fast(ScanFacts{5, 1, 96}, 16, 2, 96, 0));     // whole 128-sample pieces
    EXPECT(!scan_fast(ScanFacts{5, 1, 64}, 16, 2, 128, 0) && !scan_fast(ScanFacts{5, 1, -1}, 16, 2, 128, 0));   // G made for this chunk length
    EXPECT(!scan_fast(ok, 16, 2, 128, 1));                     // iir_no_mfma
    EXPECT(scan_fast(ScanFacts{0, 0, 256}, 2, 2, 256, 0));     // (the look-back depth is not part of it)
    EXPECT(scan_interleaved_applies(true, 128) && !scan_interleaved_applies(false, 128) && !scan_interleaved_applies(true, 96));
    EXPECT(scan_k1(false, false, 16, 128) == kK1Chunk && scan_k1(true, false, 16, 128) == kK1Regs && scan_k1(true, false, 16, 256) == kK1Regs &&
           scan_k1(true, false, 16, 512) == kK1Regs && scan_k1(true, false, 16, 384) == kK1Mfma && scan_k1(true, false, 18, 128) == kK1Mfma &&
           scan_k1(true, true, 16, 128) == kK1Mfma);
    // the single pass
    EXPECT(fused_chunk(false, false) == 128 && fused_chunk(true, false) == 64 && fused_chunk(false, true) == 64 && fused_chunk(true, true) == 32);
    const int64_t edge = (int64_t)128 * 256 * 256;
    EXPECT(fused_wanted(2, 16, 0, 0, 1, 1, false, false, edge, false, 256));
    EXPECT(!fused_wanted(2, 16, 0, 0, 1, 1, false, false, edge - 1, false, 256));           // enough segments to fill the chip
    EXPECT(fused_wanted(2, 16, 0, 0, 1, 1, false, false, edge / 2, true, 256) && !fused_wanted(2, 16, 0, 0, 1, 1, false, false, edge / 2 - 1, true, 256));
    EXPECT(fused_wanted(2, 16, 0, 0, 1, 2, true, false, edge / 2, false, 256) && !fused_wanted(2, 16, 0, 0, 1, 2, true, false, edge / 2 - 1, false, 256));
    EXPECT(fused_wanted(2, 16, 0, 0, 1, 1, false, false, edge / 2, false, 128));            // ... of this chip
    EXPECT(!fused_wanted(4, 16, 0, 0, 1, 1, false, false, edge, false, 256));               // biquads
    EXPECT(!fused_wanted(2, 18, 0, 0, 1, 1, false, false, edge, false, 256));               // at most 8 of them
    EXPECT(!fused_wanted(2, 16, 1, 0, 1, 1, false, false, edge, false, 256) && fused_wanted(2, 16, -1, 0, 1, 1, false, false, edge, false, 256));   // iir_two_pass
    EXPECT(!fused_wanted(2, 16, 0, -1, 1, 1, false, false, edge, false, 256) && fused_wanted(2, 16, 0, 1, 1, 1, false, false, edge, false, 256));   // the cached refusal
    EXPECT(fused_wanted(2, 16, 0, 0, 3, 1, false, false, edge, false, 256) && !fused_wanted(2, 16, 0, 0, 3, 1, false, true, edge, false, 256));     // .dn: no state out,
    EXPECT(!fused_wanted(2, 16, 0, 0, 3, 2, false, false, edge, false, 256) && fused_wanted(2, 16, 0, 0, 3, 2, true, false, edge, false, 256));     // one row or interleaved
    EXPECT(fused_wanted(2, 16, 0, 0, 1, 2, false, true, edge, false, 256));                 // (states and planes are fine at full rate)
    EXPECT(fused_applies(ScanFacts{6, 1, 128}, 128) && !fused_applies(ScanFacts{6, 2, 128}, 128) && !fused_applies(ScanFacts{6, 0, 128}, 128) &&
           !fused_applies(ScanFacts{6, 1, -1}, 128));
    EXPECT(fused_policy(false, false, 9, 0) && fused_policy(true, true, 9, 0) && fused_policy(true, false, 5, 0) && !fused_policy(true, false, 6, 0) &&
           fused_policy(true, false, 6, -1));
    EXPECT(scan_negl(true) == 1e-30L && scan_negl(false) == 1e-18L);
}

int main()
{
    half_pole(32);
    half_pole(128);
    slow_pole();
    block_triangular();
    geometry();
    rules();
    printf(g_fail ? "%d FAILED\n" : "OK\n", g_fail);
    return g_fail ? 1 : 0;
}
