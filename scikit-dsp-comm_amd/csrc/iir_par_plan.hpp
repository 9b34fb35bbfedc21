// iir_par_plan.hpp -- the numerical host code and the dispatch decision of the parallel-form IIR scan (iir_par.hip): the partial-fraction
// expansion of a cascade and its acceptance test, the float32 from-rest probe (V32), the values of the scan / look-back / jump tables, and
// par_choose -- which chunk length, table slot and kernel family a call gets.  Standard headers only: it compiles without a device toolchain,
// and tests/host/iir_par_plan_emul.cpp runs it on the host.  iir_par.hip keeps the kernel, the device copies of these tables and the launch.
#pragma once
#include <vector>
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>

namespace skdsp {

// the kernel's constants this code depends on (iir_par.hip ties each to its own with a static_assert)
constexpr int kParPlanMaxK = 8;         // kParMaxK: look-back depth the tables hold
constexpr int kParPlanT32 = 128;        // SK_PAR_T32: samples per chunk of float32 signals; float64 signals: half
constexpr int kParPlanStageM2 = 13312;  // kParStageM2: bytes of a wave's stage image in the DECM = 3 kernels
// bytes of a wave's stage image: 64 rows of Stage<IO>::pitch elements (iir_common.hpp: 36 floats / 34 doubles)
constexpr int64_t par_stage_image_bytes(int elem_bytes) { return elem_bytes == 4 ? (int64_t)64 * 36 * 4 : (int64_t)64 * 34 * 8; }

// H(z) = c0 + sum_k (r0_k + r1_k z^-1) / (1 + a1_k z^-1 + a2_k z^-2) of a cascade, and what the kernels run of it
struct ParExpansion {
    int nsec = 0;
    long double a1[8] = {}, a2[8] = {}, r0[8] = {}, r1[8] = {}, c0 = 0.0L;
    double na1[8] = {}, na2[8] = {}, al[8] = {}, be[8] = {}, gamma = 0.0;   // -a1, -a2; the output taps on (w[n-1], w[n-2]); the direct term
    double kappa = 0.0, ir_err = 0.0, l1h = 0.0;   // (l1h: the l1 norm of the impulse response -- the forward bound per unit input)
};

struct Q2 { long double u, v; };   // u + v q  in R[q] / (1 + a1 q + a2 q^2)

// partial fractions of prod_k B_k(q) / A_k(q), q = z^-1, by arithmetic modulo each denominator
inline bool par_expand(const double *coef, int nsec, ParExpansion &P)
{
    P.nsec = nsec;
    long double b[8][3], a[8][3];
    int degA[8], degB[8], sumA = 0, sumB = 0;
    for (int k = 0; k < nsec; ++k) {
        const double *c = coef + 5 * k;
        b[k][0] = c[0]; b[k][1] = c[1]; b[k][2] = c[2];
        a[k][0] = 1.0L; a[k][1] = c[3]; a[k][2] = c[4];
        for (int i = 0; i < 5; ++i)
            if (!std::isfinite(c[i])) return false;
        degA[k] = a[k][2] != 0.0L ? 2 : (a[k][1] != 0.0L ? 1 : 0);
        degB[k] = b[k][2] != 0.0L ? 2 : (b[k][1] != 0.0L ? 1 : 0);
        sumA += degA[k];
        sumB += degB[k];
    }
    if (sumB > sumA) return false;   // a polynomial part beyond the direct term: not a sum of these branches
    P.c0 = 0.0L;
    if (sumB == sumA) {
        P.c0 = 1.0L;
        for (int k = 0; k < nsec; ++k) P.c0 *= b[k][degB[k]] / a[k][degA[k]];
    }
    for (int k = 0; k < nsec; ++k) {
        P.a1[k] = a[k][1];
        P.a2[k] = a[k][2];
        P.r0[k] = P.r1[k] = 0.0L;
        if (degA[k] == 2) {
            const long double a1 = a[k][1], a2 = a[k][2];
            auto red = [&](const long double *c) { return Q2{c[0] - c[2] / a2, c[1] - c[2] * a1 / a2}; };
            auto mul = [&](Q2 x, Q2 y) {
                const long double vv = x.v * y.v;
                return Q2{x.u * y.u - vv / a2, x.u * y.v + x.v * y.u - vv * a1 / a2};
            };
            Q2 acc{1.0L, 0.0L};
            for (int jx = 0; jx < nsec; ++jx) {
                acc = mul(acc, red(b[jx]));
                if (jx == k) continue;
                const Q2 d = red(a[jx]);
                // inverse of d: [u, -v/a2; v, u - v a1/a2] [s; t] = [1; 0]
                const long double m11 = d.u, m12 = -d.v / a2, m21 = d.v, m22 = d.u - d.v * a1 / a2;
                const long double det = m11 * m22 - m12 * m21;
                const long double scale = fabsl(m11 * m22) + fabsl(m12 * m21);
                if (!(fabsl(det) > 1e-12L * scale) || !std::isfinite((double)det)) return false;   // a pole shared with another section
                acc = mul(acc, Q2{m22 / det, -m21 / det});
            }
            P.r0[k] = acc.u;
            P.r1[k] = acc.v;
        } else if (degA[k] == 1) {
            const long double q0 = -1.0L / a[k][1];
            long double val = 1.0L;
            for (int jx = 0; jx < nsec; ++jx) {
                val *= b[jx][0] + b[jx][1] * q0 + b[jx][2] * q0 * q0;
                if (jx == k) continue;
                const long double den = a[jx][0] + a[jx][1] * q0 + a[jx][2] * q0 * q0;
                if (!(fabsl(den) > 1e-12L)) return false;
                val /= den;
            }
            P.r0[k] = val;
        }
        if (!std::isfinite((double)P.r0[k]) || !std::isfinite((double)P.r1[k])) return false;
    }
    if (!std::isfinite((double)P.c0)) return false;
    long double gam = P.c0;
    for (int k = 0; k < nsec; ++k) {
        P.na1[k] = (double)(-P.a1[k]);
        P.na2[k] = (double)(-P.a2[k]);
        P.al[k] = (double)(P.r1[k] - P.r0[k] * P.a1[k]);
        P.be[k] = (double)(-P.r0[k] * P.a2[k]);
        gam += P.r0[k];
    }
    P.gamma = (double)gam;
    // acceptance: the expansion with its double coefficients against the cascade (long double DF2T), impulse response
    const int NI = 8192;
    long double zc[16] = {0}, w1[8] = {0}, w2[8] = {0};
    long double hmax = 0.0L, emax = 0.0L, l1h = 0.0L, l1b = fabsl((long double)P.gamma);
    for (int n = 0; n < NI; ++n) {
        long double xin = n == 0 ? 1.0L : 0.0L, xc = xin;
        for (int s = 0; s < nsec; ++s) {
            const double *c = coef + 5 * s;
            const long double yv = (long double)c[0] * xc + zc[2 * s];
            zc[2 * s] = (long double)c[1] * xc - (long double)c[3] * yv + zc[2 * s + 1];
            zc[2 * s + 1] = (long double)c[2] * xc - (long double)c[4] * yv;
            xc = yv;
        }
        long double yp = (long double)P.gamma * xin;
        for (int s = 0; s < nsec; ++s) {
            const long double br = (long double)P.al[s] * w1[s] + (long double)P.be[s] * w2[s];
            yp += br;
            if (n > 0) l1b += fabsl(br);
            const long double w0 = xin + (long double)P.na1[s] * w1[s] + (long double)P.na2[s] * w2[s];
            w2[s] = w1[s];
            w1[s] = w0;
        }
        hmax = std::max(hmax, fabsl(xc));
        emax = std::max(emax, fabsl(xc - yp));
        l1h += fabsl(xc);
    }
    if (!(hmax > 0.0L) || !std::isfinite((double)emax) || !std::isfinite((double)l1b)) return false;
    P.ir_err = (double)(emax / hmax);
    P.kappa = (double)(l1b / l1h);
    P.l1h = (double)l1h;
    return P.ir_err <= 1e-12 && P.kappa <= 1e3;
}

// V32 (see the kernel): may the from-rest end states of T-sample chunks of THIS filter be formed in float32?  The error such a state carries reaches the
// outputs of the next chunks through the output taps, amplified by whatever cancels between the branches -- no norm of the expansion predicts it (an
// elliptic band-pass with a cancellation factor of 2.8 shows 1.6e-6, one with 3.7 shows 4e-7), so it is MEASURED by a model of the kernel: the float32
// chain of the matrix instruction (acc = fmaf(G[t], x[t], acc), oldest sample first, G rounded to float32 -- bit for bit what v_mfma_f32_16x16x4_f32
// computes) against the exact from-rest state; the state errors are carried from chunk to chunk by the exact transition and through the output taps
// sample by sample.  par_v32_input_error is the model on one input, par_v32_probe the admission test: the model on a fixed set of inputs.

// the table G of T-sample chunks as the float32 kernel holds it (g32) and unrounded (gd): rows 2k, 2k + 1 are g[T-1-t], g[T-2-t], g = impulse response of 1 / A_k
struct ParV32G {
    int T = 0;
    std::vector<float> g32;
    std::vector<double> gd;
};
inline ParV32G par_v32_g(const ParExpansion &P, int T)
{
    const int N = P.nsec;
    ParV32G G;
    G.T = T;
    G.g32.resize((size_t)2 * N * T);
    G.gd.resize((size_t)2 * N * T);
    for (int k = 0; k < N; ++k) {
        long double g0 = 1.0L, g1 = 0.0L;
        for (int t = T - 1; t >= 0; --t) {
            G.gd[((size_t)2 * k) * T + t] = (double)g0;
            G.gd[((size_t)2 * k + 1) * T + t] = (double)g1;
            G.g32[((size_t)2 * k) * T + t] = (float)(double)g0;
            G.g32[((size_t)2 * k + 1) * T + t] = (float)(double)g1;
            const long double g2 = -P.a1[k] * g0 - P.a2[k] * g1;
            g1 = g0;
            g0 = g2;
        }
    }
    return G;
}

// The model on ONE input: x holds nch chunks of G.T samples.  Returned: the worst output error the float32 from-rest states cause on it, over the scale
// (the input's exact output peak, or 1 % of the forward bound); infinity where there is nothing to scale by.  State errors only: the recurrence and the
// output rounding of the kernel are not in it.
inline double par_v32_input_error(const ParExpansion &P, const ParV32G &G, const float *x, int nch)
{
    const int N = P.nsec, T = G.T, n = nch * T;
    // the exact output (the parallel form in double, straight through) for the scale; the error by linearity: the state errors alone, carried exactly
    double ymax = 0.0, xmax = 0.0;
    {
        std::vector<double> w1((size_t)N, 0.0), w2((size_t)N, 0.0);
        for (int i = 0; i < n; ++i) {
            double yv = P.gamma * (double)x[i];
            for (int k = 0; k < N; ++k) {
                yv += P.al[k] * w1[k] + P.be[k] * w2[k];
                const double w0 = (double)x[i] + P.na1[k] * w1[k] + P.na2[k] * w2[k];
                w2[k] = w1[k];
                w1[k] = w0;
            }
            ymax = std::max(ymax, std::fabs(yv));
            xmax = std::max(xmax, (double)std::fabs(x[i]));
        }
    }
    std::vector<double> e1((size_t)N, 0.0), e2((size_t)N, 0.0);   // error of (w[n-1], w[n-2]) at the start of the current chunk
    double emax = 0.0;
    for (int j = 0; j < nch; ++j) {
        // outputs of chunk j see the start-state error through the taps; the error state runs the homogeneous recurrence
        std::vector<double> f1 = e1, f2 = e2;
        for (int t = 0; t < T; ++t) {
            double ev = 0.0;
            for (int k = 0; k < N; ++k) {
                ev += P.al[k] * f1[k] + P.be[k] * f2[k];
                const double f0 = P.na1[k] * f1[k] + P.na2[k] * f2[k];
                f2[k] = f1[k];
                f1[k] = f0;
            }
            emax = std::max(emax, std::fabs(ev));
        }
        // this chunk's from-rest end state: the float32 chain against the double sum of the same products with the unrounded G
        for (int k = 0; k < N; ++k) {
            for (int c = 0; c < 2; ++c) {
                const float *gf = G.g32.data() + ((size_t)2 * k + c) * T;
                const double *ge = G.gd.data() + ((size_t)2 * k + c) * T;
                float acc = 0.0f;
                long double ex = 0.0L;
                for (int t = 0; t < T; ++t) {
                    acc = std::fmaf(gf[t], x[(size_t)j * T + t], acc);
                    ex += (long double)ge[t] * (long double)x[(size_t)j * T + t];
                }
                (c == 0 ? f1[k] : f2[k]) += (double)acc - (double)ex;   // e_(j+1) = Phi e_j + delta_j (f holds Phi e_j now)
            }
        }
        e1 = f1;
        e2 = f2;
    }
    const double scale = std::max(ymax, 1e-2 * P.l1h * xmax);
    if (!(scale > 0.0) || !std::isfinite(emax)) return HUGE_VAL;
    return emax / scale;
}
inline double par_v32_input_error(const ParExpansion &P, int T, const float *x, int nch) { return par_v32_input_error(P, par_v32_g(P, T), x, nch); }

// the resonance angle of section k (complex poles), or a negative value: real poles -- DC / Nyquist cover them
inline double par_resonance(const ParExpansion &P, int k)
{
    const double a1 = (double)P.a1[k], a2 = (double)P.a2[k];
    if (!(a2 > 0.0) || a1 * a1 >= 4.0 * a2) return -1.0;
    return std::acos(std::max(-1.0, std::min(1.0, -a1 / (2.0 * std::sqrt(a2)))));
}

// the probe's noise: sums of four uniform draws of a fixed generator, unit variance
inline void par_v32_noise(float *x, int n)
{
    unsigned long long lcg = 0x2545F4914F6CDD1Dull;
    for (int i = 0; i < n; ++i) {
        double a = 0.0;
        for (int q = 0; q < 4; ++q) {
            lcg = lcg * 6364136223846793005ull + 1442695040888963407ull;
            a += (double)(lcg >> 11) / 9007199254740992.0 - 0.5;
        }
        x[i] = (float)(a * 1.7320508075688772);
    }
}

// The admission test: the worst model error over noise, DC, the Nyquist alternation and, for every section with complex poles, tones ON its resonance
// (cosine and sine phase) and DETUNED from it by +- 0.005, 0.015 and 0.03 rad / sample, 96 chunks each.  The detuned tones are the ones that decide: just
// outside a band edge the states of the edge sections are still as large as on the resonance while the output -- the scale -- has fallen to a fraction,
// and a tone that is not periodic in the chunk length meets every phase of the chunk grid, which takes some tens of chunks (measured, model and GPU,
// BASELINE config 4 shows 4.0e-7 on its resonances over 24 chunks, 1.33e-6 at 0.009 rad above its upper edge resonance over 96
// and 1.37e-6 over 512; the GPU 1.46e-6).  Over a 0.001 rad grid of +- 0.03 around every resonance, square waves, combs and zero-stuffed tones the model
// stays within 1.5 times this probe's value for every cascade the probe admits (tests/host/iir_par_v32_emul.cpp holds it to that).
// Returned: the worst error over scale; 1.0 where an input has nothing to scale by.  stop_above: the inputs after the first one that shows more than this
// are not run (the launch passes kParV32Limit: a refusal needs no more than one such input, and the whole set costs 0.1 - 0.2 s for 8 biquads).
constexpr int kParV32ProbeChunks = 96;
constexpr double kParV32Detune[3] = {0.005, 0.015, 0.03};
inline double par_v32_probe(const ParExpansion &P, int T, double stop_above = HUGE_VAL)
{
    const int N = P.nsec, NCH = kParV32ProbeChunks, n = NCH * T;
    const ParV32G G = par_v32_g(P, T);
    std::vector<float> x((size_t)n);
    double worst = 0.0;
    auto run = [&]() {
        const double e = par_v32_input_error(P, G, x.data(), NCH);
        worst = std::max(worst, e);
        return std::isfinite(e);
    };
    auto done = [&]() { return worst > stop_above; };
    auto tone = [&](double w) {
        for (int i = 0; i < n; ++i) x[i] = (float)std::cos(w * i);
        return run();
    };
    par_v32_noise(x.data(), n);
    if (!run()) return 1.0;
    for (int i = 0; i < n; ++i) x[i] = 1.0f;
    if (!run()) return 1.0;
    for (int i = 0; i < n; ++i) x[i] = (i & 1) ? -1.0f : 1.0f;
    if (!run()) return 1.0;
    // (the sections with the sharpest poles first: where a filter is refused, it is mostly next to those)
    int order[8] = {0, 1, 2, 3, 4, 5, 6, 7};
    std::stable_sort(order, order + N, [&](int a, int b) { return P.a2[a] > P.a2[b]; });
    for (int ko = 0; ko < N && !done(); ++ko) {
        const int k = order[ko];
        const double th = par_resonance(P, k);
        if (th < 0.0) continue;
        if (!tone(th)) return 1.0;
        for (int i = 0; i < n; ++i) x[i] = (float)std::sin(th * i);
        if (!run()) return 1.0;
        for (double d : kParV32Detune)
            for (double w : {th - d, th + d})
                if (w > 0.0 && w < 3.141592653589793 && !done() && !tone(w)) return 1.0;
    }
    return worst;
}
constexpr double kParV32Limit = 5e-7;   // of the 1e-6 the float32 contract allows: the rest stays with the recurrence, the output rounding and the inputs no probe covers
// ... of which the kernel with float64 from-rest states (recurrence, output rounding) takes this much: the largest error tests/test_gpu_iir_v32.py records
// with iir_par_v32 = 0 on its designs' resonance and worst detuned tones (MI355X, 49152 samples, 15 cascades the parallel form serves, float32 and complex64,
// .filter / .dn / .up: 5.0e-8 ... 6.7e-8), rounded up.  tests/host/iir_par_v32_emul.cpp holds the model to 1e-6 minus this.
constexpr double kParV32Rest = 1e-7;

struct M2 { long double m[4]; };
inline M2 m2mul(const M2 &x, const M2 &y)
{
    return M2{{x.m[0] * y.m[0] + x.m[1] * y.m[2], x.m[0] * y.m[1] + x.m[1] * y.m[3], x.m[2] * y.m[0] + x.m[3] * y.m[2],
               x.m[2] * y.m[1] + x.m[3] * y.m[3]}};
}
inline long double m2max(const M2 &x) { return std::max(std::max(fabsl(x.m[0]), fabsl(x.m[1])), std::max(fabsl(x.m[2]), fabsl(x.m[3]))); }

// The tables of one (chunk length T, chunks per wave segment) pair, as host values.  negl: the negligibility threshold -- 1e-30 for float64 signals,
// 1e-18 for float32 ones, as in iir_scan.hip (a tenth of an ulp of the float64 state the dropped term would be added to)
struct ParTableValues {
    std::vector<double> gt;    // G in MFMA A-operand order [T / 4][64]
    std::vector<double> lvl;   // Phi^(2^l), l = 0..5: [6][nsec][4]
    std::vector<double> psi;   // Psi^m, m = 1..kParPlanMaxK-1, Psi = Phi^(chunks per segment): [kParPlanMaxK - 1][nsec][4]
    int n_lv = 0, K = 0;       // scan levels that matter; look-back depth
    bool failed = false;       // a power is not finite, or the filter remembers more than kmax segments of this length (K = 0: not served)
};

inline ParTableValues par_table_values(const ParExpansion &P, int T, int chunks, long double negl, int kmax)
{
    const int LV = chunks == 64 ? 6 : 5;   // scan levels inside a wave segment of `chunks` chunks
    const int N = P.nsec;
    ParTableValues v;
    v.failed = true;
    std::vector<double> &lvl = v.lvl, &psi = v.psi, &gt = v.gt;
    lvl.assign((size_t)6 * N * 4, 0.0);
    psi.assign((size_t)(kParPlanMaxK - 1) * N * 4, 0.0);
    gt.assign((size_t)T * 16, 0.0);
    long double lvmax[7] = {0}, psimax[kParPlanMaxK + 1] = {0};
    for (int k = 0; k < N; ++k) {
        // one-sample zero-input transition of (w[n-1], w[n-2]);  Phi = its T-th power
        M2 one{{-P.a1[k], -P.a2[k], 1.0L, 0.0L}}, Phi{{1.0L, 0.0L, 0.0L, 1.0L}}, sq = one;
        for (int e = T; e; e >>= 1) {
            if (e & 1) Phi = m2mul(Phi, sq);
            sq = m2mul(sq, sq);
        }
        M2 pw = Phi;
        for (int l = 0; l <= LV; ++l) {
            lvmax[l] = std::max(lvmax[l], m2max(pw));
            if (!std::isfinite((double)m2max(pw))) return v;
            if (l < LV)
                for (int i = 0; i < 4; ++i) lvl[((size_t)l * N + k) * 4 + i] = (double)pw.m[i];
            if (l < LV) pw = m2mul(pw, pw);
        }
        const M2 Psi = pw;   // Phi^chunks: the transition over one wave segment
        M2 pk = Psi;
        for (int m = 1; m <= kParPlanMaxK; ++m) {
            psimax[m] = std::max(psimax[m], m2max(pk));
            if (m < kParPlanMaxK)
                for (int i = 0; i < 4; ++i) psi[((size_t)(m - 1) * N + k) * 4 + i] = (double)pk.m[i];
            pk = m2mul(pk, Psi);
        }
        // G rows 2k, 2k+1: g[T-1-t], g[T-2-t], g = impulse response of 1 / A_k; as the MFMA A operand of step t / 4:
        // lane l holds row l & 15, column 4 (t / 4) + (l >> 4)
        long double g0 = 1.0L, g1 = 0.0L;   // g[i], g[i-1]
        for (int t = T - 1; t >= 0; --t) {
            const size_t at = (size_t)(t / 4) * 64 + (size_t)(t % 4) * 16;
            gt[at + 2 * k] = (double)g0;
            gt[at + 2 * k + 1] = (double)g1;
            const long double g2 = -P.a1[k] * g0 - P.a2[k] * g1;
            g1 = g0;
            g0 = g2;
        }
    }
    v.n_lv = LV;
    for (int l = LV; l >= 0; --l)
        if (lvmax[l] < negl) v.n_lv = std::min(v.n_lv, l);
    v.K = 0;
    for (int m = 1; m <= kmax; ++m)
        if (psimax[m] < negl) { v.K = m; break; }
    if (v.K == 0) return v;   // remembers more than kmax segments
    if (v.n_lv < LV) v.K = 1;
    v.failed = false;
    return v;
}

// UPJ table of an expansion for the factor L (see the kernel): rows c A^j, j = 0 .. L - 1, c = (al, be) of every section; then the 2 x 2 blocks of A^L
inline std::vector<double> par_upj_values(const ParExpansion &P, int L)
{
    const int N = P.nsec, D = 2 * N;
    // layout: rows 0 .. L - 1; up to 4 biquads (the kernels that read rows in pairs) row 0 once more; the blocks of A^L
    const size_t rows = (size_t)L + (N <= 4 ? 1 : 0);
    std::vector<double> tab(rows * D + (size_t)N * 4);
    for (int k = 0; k < N; ++k) {
        const long double A[4] = {-P.a1[k], -P.a2[k], 1.0L, 0.0L};   // (w[n-1], w[n-2]) -> (w[n], w[n-1]) without input
        long double c0 = (long double)P.al[k], c1 = (long double)P.be[k];   // the row c A^j
        long double M[4] = {1.0L, 0.0L, 0.0L, 1.0L};                  // A^j
        for (int j = 0; j < L; ++j) {
            tab[(size_t)j * D + 2 * k] = (double)c0;
            tab[(size_t)j * D + 2 * k + 1] = (double)c1;
            const long double n0 = c0 * A[0] + c1 * A[2], n1 = c0 * A[1] + c1 * A[3];
            c0 = n0; c1 = n1;
            const long double m0 = M[0] * A[0] + M[1] * A[2], m1 = M[0] * A[1] + M[1] * A[3], m2 = M[2] * A[0] + M[3] * A[2], m3 = M[2] * A[1] + M[3] * A[3];
            M[0] = m0; M[1] = m1; M[2] = m2; M[3] = m3;
        }
        if (N <= 4) {
            tab[(size_t)L * D + 2 * k] = tab[2 * k];
            tab[(size_t)L * D + 2 * k + 1] = tab[2 * k + 1];
        }
        for (int i = 0; i < 4; ++i) tab[rows * D + 4 * k + i] = (double)M[i];   // A^L
    }
    return tab;
}

// .dn: can a segment's kept outputs be gathered in the wave's stage image (see ParArgs::dec_compact)?
// (lean: the 96-sample kernels put a kept output into its slot straight from the sum -- no unit to pick it from, so M may be below the samples of a unit)
inline bool par_dec_compact(int elem_bytes, bool cplx, int dec, int64_t seg_samples, bool lean, int64_t image_bytes, int iir_dn_compact)
{
    const int elems = 16 / elem_bytes, ls = cplx ? 2 : 1;
    const int64_t slots = (seg_samples / dec + 2) * ls;
    const int64_t bytes = (slots + slots / 32 + 2) * (int64_t)elem_bytes;
    return (lean || dec >= elems) && bytes <= (image_bytes ? image_bytes : par_stage_image_bytes(elem_bytes)) && iir_dn_compact;
}

// .dn with dec below the samples of a 16-byte unit (float32 / complex64, dec = 2, 3): gathered in two ranges of chunks behind the recurrence
inline bool par_dec_rounds(int elem_bytes, int dec, int iir_dn_compact) { return elem_bytes == 4 && (dec == 2 || dec == 3) && iir_dn_compact; }

// ----------------------------------------------------------------------------------------------------------- the dispatch decision
struct ParOptions { int iir_dn_t96, iir_up_jump, iir_up_lean, iir_dn_compact, iir_par_v32; };   // the run-time switches par_choose reads (skdsp_internal.hpp: Options)

// table slots of a plan: [0] float32 (T = 128), [1] float64 (T = 64), [2] complex64, [3] complex128 (32 chunks per segment),
// [4] / [5] float32 / complex64 with T = 96 (.dn, .up), [6] / [7] float64 / complex128 with T = 96 (.up)
constexpr bool par_slot_dbl(int slot) { return slot < 4 ? (slot & 1) != 0 : slot >= 6; }
constexpr bool par_slot_cplx(int slot) { return slot < 4 ? slot >= 2 : (slot & 1) != 0; }
constexpr int par_slot_T(int slot) { return slot >= 4 ? 96 : (par_slot_dbl(slot) ? kParPlanT32 / 2 : kParPlanT32); }
constexpr int par_slot_chunks(int slot) { return par_slot_cplx(slot) ? 32 : 64; }
constexpr long double par_slot_negl(int slot) { return par_slot_dbl(slot) ? 1e-30L : 1e-18L; }

struct ParChoice {
    int status = 1;            // 0: served as below; 1: the parallel form does not take this call; < 0: the K query failed with this code
    int slot = 0;              // table slot 0..7
    int TT = 0;                // the kernel family <TT, UPJ, UPS> ...
    bool UPJ = false;
    int UPS = 0;
    int DECM = 0;              // ... and the variant inside it
    bool dec_compact = false;  // ParArgs::dec_compact, dec_rounds
    int dec_rounds = 1;
    bool v32_wanted = false;   // V32 applies to this call IF the slot's probe admits the filter (or iir_par_v32 = 2): the probe runs only then
};

// the shape of a call the parallel form takes at all (before any plan exists)
inline bool par_call_shape_ok(int nsec, bool interleaved, int nrow, int dec, int up, int64_t n)
{
    if (interleaved && nrow != 1) return false;
    // .up: x holds n / up samples; one row, no decimation; the exact-division trick of the staging covers up <= 4096
    if (up > 1 && (dec > 1 || nrow != 1 || up > 4096 || n % up != 0)) return false;
    return nsec >= 1 && nsec <= 8;
}

// Which tables and which kernel a call gets.  k_of(slot): the look-back depth K of that table slot (0: the filter remembers more segments of that
// length than the look-back serves; < 0: an error) -- asked only for the slots the decision depends on, in the order the tables are made.
template <typename KQuery>
inline ParChoice par_choose(int nsec, bool dbl, bool interleaved, int nrow, int dec, int up, int64_t n, const ParOptions &o, KQuery &&k_of)
{
    ParChoice c;
    if (!par_call_shape_ok(nsec, interleaved, nrow, dec, up, n)) return c;
    const int eb = dbl ? 8 : 4, il = interleaved ? 1 : 0;
    const int64_t chunks = interleaved ? 32 : 64;
    // .dn of float32 / complex64 signals by a divisor of 96: chunks of 96 samples, so that all lanes of a wave walk the same phase (see the kernel).
    // From M = 4 on the 96-sample kernel is the compact store in its lean form (DNL in the kernel: which samples are kept is wave-uniform).  Measured, 2^26 inputs
    // (_var/dn_t96.py, profiles/r05/iir_dn_lean.txt): order-8 Butterworth M = 4 .. 96 float32 0.105 - 0.122 -> 0.086 - 0.099 ms, complex64 0.198 - 0.223 -> 0.172 - 0.196;
    // 8 biquads: float32 - 3 .. - 6 %, complex64 - 3 % where 3 divides M (128-sample chunks then start on three phases) and + 4 .. + 7 % elsewhere.
    // Before the lean form: M = 2, 3, 6 only (M = 3 0.193 -> 0.173 ms, M = 4 + 7 .. 9 %).  Option iir_dn_t96 = 2: every divisor of 96; 0: never.
    const bool t96_pays = dec == 2 || dec == 3 || dec == 6 || (96 % dec == 0 && (nsec <= 4 || !interleaved || dec % 3 == 0));
    bool t96 = !dbl && dec > 1 && (((o.iir_dn_t96 == 1 || o.iir_dn_t96 == 3) && t96_pays) || (o.iir_dn_t96 == 2 && 96 % dec == 0));
    // (the 96-sample kernels have no store but the gathering ones: the lean compact store where a segment's kept outputs fit the image -- from M = 3 on --, ranges of chunks for M = 2)
    if (t96 && !(par_dec_compact(4, interleaved, dec, chunks * 96, true, 0, o.iir_dn_compact) || par_dec_rounds(4, dec, o.iir_dn_compact))) t96 = false;
    // .up by a divisor of 96 from 8 on (the reference default 12): the lean kernels whose state jumps from input sample to input sample (UPJ, chunks of 96 so
    // that every chunk starts on one).  Measured, same box (profiles/r05/iir_up_lean.txt): rate_change(12).up float32 0.101 -> 0.072 ms per 2^26 outputs; 8-biquad
    // elliptic by 12 0.113 -> 0.092 per 5e7 (complex64 0.216 -> 0.183); 5 biquads by 8 0.132 -> 0.096 (0.231 -> 0.164).  Option iir_up_jump = 0: never
    const bool upj = dec <= 1 && up >= 8 && 96 % up == 0 && o.iir_up_jump >= 1;
    // .up by 3 (a stage of sigsys.interp24): the lean staging at the input rate (UPS in the kernel), on chunks of 96
    const bool ups3 = !dbl && dec <= 1 && up == 3 && o.iir_up_lean;   // (float64: four images of 96 doubles per row and the table leave room for ONE workgroup per CU)
    t96 = t96 || upj || ups3;
    if (t96) {
        const int K = k_of((dbl ? 6 : 4) + il);
        if (K < 0) { c.status = K; return c; }
        if (K == 0) t96 = false;   // (the filter remembers more segments of this length than the look-back serves: the 128-sample chunks, if they do)
    }
    if (t96 && upj) {
        c.slot = (dbl ? 6 : 4) + il; c.TT = 96; c.UPJ = true;
    } else if (t96 && ups3) {
        c.slot = 4 + il; c.TT = 96; c.UPS = 3;
    } else {
        if (upj || ups3) t96 = false;
        c.slot = t96 ? 4 + il : (dbl ? 1 : 0) + (interleaved ? 2 : 0);
        const int K = k_of(c.slot);
        if (K < 0) { c.status = K; return c; }
        if (K == 0) return c;
        // (interleaved signals have no decimating store here but the compact one)
        const int64_t seg = (int64_t)32 * par_slot_T(c.slot);
        if (interleaved && dec > 1 && !(dbl ? par_dec_compact(8, true, dec, seg, false, 0, o.iir_dn_compact)
                                            : (par_dec_compact(4, true, dec, seg, false, 0, o.iir_dn_compact) || par_dec_rounds(4, dec, o.iir_dn_compact)))) return c;
        // .up by 2 / 4 (where the state jump does not pay; with 3 above, the stages of sigsys.interp24): staged at the input rate, the stuffed zeros known to the
        // compiler (UPS in the kernel).  Measured (profiles/r05/iir_up_lean.txt); option iir_up_lean = 0: the zero-stuffed image as for every other factor
        if (t96) c.TT = 96;
        else if (up == 2 && dec <= 1 && o.iir_up_lean) c.UPS = 2;
        else if (up == 4 && dec <= 1 && !dbl && o.iir_up_lean) c.UPS = 4;   // (a float64 chunk of 64 holds 16 inputs: half a staging piece)
    }
    // the variant: how a decimating call stores, and whether the float32 from-rest states may apply
    const int adec = dec > 1 ? dec : 1;
    const int64_t S = chunks * par_slot_T(c.slot);   // samples per wave segment
    // (M = 2 on 96-sample chunks, more than 4 biquads, float32 / complex64: the DECM = 3 kernels with their larger image)
    const bool big_m2 = c.TT == 96 && eb == 4 && !c.UPJ && c.UPS == 0 && adec == 2 && nsec > 4 && o.iir_dn_t96 != 3;
    c.dec_compact = adec > 1 && par_dec_compact(eb, interleaved, adec, S, c.TT == 96, big_m2 ? kParPlanStageM2 : 0, o.iir_dn_compact);
    c.dec_rounds = !c.dec_compact && par_dec_rounds(eb, adec, o.iir_dn_compact) ? 2 : 1;
    c.DECM = adec <= 1 ? 0 : c.dec_rounds > 1 ? 2 : (big_m2 && c.dec_compact) ? 3 : 1;
    // V32 (see the kernel): float32 / complex64 signals through 7 - 8 biquads, .filter and .up.  Not .dn: the contract is relative to the peak of the outputs a call
    // KEEPS, and every M-th sample of a tone can peak far below the tone -- the probe's scale is the full-rate peak, and a state error it admits at 4.4e-7 of that
    // measured 1.6e-6 of the kept outputs' peak (an 8-band equaliser, sine on its lowest resonance, .dn(x, 5)); the float64 states (6e-8) have the room for that
    // (not for .up by 8 or more through the general kernel: its from-rest states are formed per lane on the vector ALU from the FLOAT64 table -- `sparse` in the kernel)
    c.v32_wanted = eb == 4 && !c.UPJ && nsec >= 7 && o.iir_par_v32 > 0 && !(c.UPS == 0 && up >= 8) && dec <= 1;
    c.status = 0;
    return c;
}

}  // namespace skdsp
