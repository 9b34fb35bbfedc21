// iir_design.hpp -- the numerical host code of IIR handle creation: (b, a) -> second-order sections, and the probes that
// decide how a cascade runs (iir_api.hip: iir_create_common).  Standard headers only: it compiles without a device
// toolchain, and tests/host/iir_design_emul.cpp runs it on the host.
#pragma once
#include <vector>
#include <complex>
#include <array>
#include <algorithm>
#include <cmath>

namespace skdsp {

// ---------------------------------------------------------------------------
// (b, a) -> cascaded biquads.  scipy.signal.lfilter runs a transfer function as ONE
// direct-form-II-transposed section of order N.  In those state coordinates the
// one-chunk transition matrix A^T of a narrow-band design (rate_change(12): Butterworth
// order 8, cutoff 0.075) has entries ~1e6 that cancel, so the affine scan would lose
// ~1e-4 of the output even in float64 (measured).  The scan therefore runs the SAME
// transfer function as second-order sections, whose state coordinates are benign; the
// result differs from the reference's TF-form recursion by its own float64 roundoff
// level (~1e-9 relative for rate_change(12), tests/golden/g8).  Conjugate pairs are
// symmetrised so every section has real coefficients.
typedef std::complex<long double> cld;

// Roots of c[0] z^n + ... + c[n] as the eigenvalues of the (real) companion matrix by
// the Francis double-shift QR iteration (the classical EISPACK "hqr" scheme) in long
// double.  Orthogonal similarity transforms are backward stable, and REAL arithmetic
// returns exactly conjugate pairs -- both matter for the N-fold zero at z = -1 of a
// Butterworth numerator: the individual roots scatter by eps^(1/N), yet the product of
// the resulting real quadratic factors reproduces the coefficients to ~1e-18 (an
// Aberth iteration, or a complex-shift QR followed by symmetrising the pairs, measured
// 1e-6 .. 1e-4 there).
static inline long double sign_ld(long double a, long double b) { return b >= 0.0L ? fabsl(a) : -fabsl(a); }

static bool poly_roots(const std::vector<long double> &c, std::vector<cld> &roots)
{
    const int n = (int)c.size() - 1;
    roots.clear();
    if (n <= 0) return true;
    std::vector<long double> A((size_t)n * n, 0.0L);
    auto a = [&](int i, int j) -> long double & { return A[(size_t)i * n + j]; };
    for (int j = 0; j < n; ++j) a(0, j) = -c[j + 1] / c[0];
    for (int i = 1; i < n; ++i) a(i, i - 1) = 1.0L;
    roots.assign(n, cld(0.0L, 0.0L));
    long double anorm = 0.0L;
    for (int i = 0; i < n; ++i)
        for (int j = (i > 0 ? i - 1 : 0); j < n; ++j) anorm += fabsl(a(i, j));
    int nn = n - 1;
    long double t = 0.0L, p = 0, q = 0, r = 0, s = 0, w = 0, x = 0, y = 0, z = 0;
    while (nn >= 0) {
        int its = 0, l;
        do {
            for (l = nn; l >= 1; --l) {
                s = fabsl(a(l - 1, l - 1)) + fabsl(a(l, l));
                if (s == 0.0L) s = anorm;
                if (fabsl(a(l, l - 1)) + s == s) { a(l, l - 1) = 0.0L; break; }
            }
            x = a(nn, nn);
            if (l == nn) {  // one root
                roots[nn--] = cld(x + t, 0.0L);
            } else {
                y = a(nn - 1, nn - 1);
                w = a(nn, nn - 1) * a(nn - 1, nn);
                if (l == nn - 1) {  // two roots
                    p = 0.5L * (y - x);
                    q = p * p + w;
                    z = sqrtl(fabsl(q));
                    x += t;
                    if (q >= 0.0L) {
                        z = p + sign_ld(z, p);
                        roots[nn - 1] = roots[nn] = cld(x + z, 0.0L);
                        if (z != 0.0L) roots[nn] = cld(x - w / z, 0.0L);
                    } else {
                        roots[nn - 1] = cld(x + p, z);
                        roots[nn] = cld(x + p, -z);
                    }
                    nn -= 2;
                } else {  // no roots yet: one double-shift sweep
                    if (its == 120) return false;
                    if (its % 10 == 0 && its > 0) {  // exceptional shift
                        t += x;
                        for (int i = 0; i <= nn; ++i) a(i, i) -= x;
                        s = fabsl(a(nn, nn - 1)) + fabsl(a(nn - 1, nn - 2));
                        y = x = 0.75L * s;
                        w = -0.4375L * s * s;
                    }
                    ++its;
                    int m;
                    for (m = nn - 2; m >= l; --m) {
                        z = a(m, m);
                        r = x - z;
                        s = y - z;
                        p = (r * s - w) / a(m + 1, m) + a(m, m + 1);
                        q = a(m + 1, m + 1) - z - r - s;
                        r = a(m + 2, m + 1);
                        s = fabsl(p) + fabsl(q) + fabsl(r);
                        p /= s; q /= s; r /= s;
                        if (m == l) break;
                        const long double u = fabsl(a(m, m - 1)) * (fabsl(q) + fabsl(r));
                        const long double v = fabsl(p) * (fabsl(a(m - 1, m - 1)) + fabsl(z) + fabsl(a(m + 1, m + 1)));
                        if (u + v == v) break;
                    }
                    for (int i = m + 2; i <= nn; ++i) {
                        a(i, i - 2) = 0.0L;
                        if (i != m + 2) a(i, i - 3) = 0.0L;
                    }
                    for (int k = m; k <= nn - 1; ++k) {
                        if (k != m) {
                            p = a(k, k - 1);
                            q = a(k + 1, k - 1);
                            r = 0.0L;
                            if (k != nn - 1) r = a(k + 2, k - 1);
                            if ((x = fabsl(p) + fabsl(q) + fabsl(r)) != 0.0L) { p /= x; q /= x; r /= x; }
                        }
                        if ((s = sign_ld(sqrtl(p * p + q * q + r * r), p)) != 0.0L) {
                            if (k == m) {
                                if (l != m) a(k, k - 1) = -a(k, k - 1);
                            } else {
                                a(k, k - 1) = -s * x;
                            }
                            p += s;
                            x = p / s; y = q / s; z = r / s;
                            q /= p; r /= p;
                            for (int j = k; j <= nn; ++j) {
                                p = a(k, j) + q * a(k + 1, j);
                                if (k != nn - 1) { p += r * a(k + 2, j); a(k + 2, j) -= p * z; }
                                a(k + 1, j) -= p * y;
                                a(k, j) -= p * x;
                            }
                            const int mmin = nn < k + 3 ? nn : k + 3;
                            for (int i = l; i <= mmin; ++i) {
                                p = x * a(i, k) + y * a(i, k + 1);
                                if (k != nn - 1) { p += z * a(i, k + 2); a(i, k + 2) -= p * r; }
                                a(i, k + 1) -= p * q;
                                a(i, k) -= p;
                            }
                        }
                    }
                }
            }
        } while (l < nn - 1);
    }
    for (auto &rt : roots)
        if (!std::isfinite((double)rt.real()) || !std::isfinite((double)rt.imag())) return false;
    return true;
}

// group roots of a real polynomial into real quadratic factors 1 + c1 z^-1 + c2 z^-2
static bool quad_factors(std::vector<cld> roots, std::vector<std::pair<long double, long double>> &quads)
{
    quads.clear();
    std::vector<cld> up, dn;
    std::vector<long double> re;
    for (auto &r : roots) {
        const long double tol = 1e-13L * (1.0L + std::abs(r));
        if (r.imag() > tol) up.push_back(r);
        else if (r.imag() < -tol) dn.push_back(r);
        else re.push_back(r.real());
    }
    if (up.size() != dn.size()) return false;
    for (auto &u : up) {
        // nearest partner to conj(u)
        size_t best = 0;
        long double bd = -1.0L;
        for (size_t j = 0; j < dn.size(); ++j) {
            const long double d = std::abs(std::conj(u) - dn[j]);
            if (bd < 0.0L || d < bd) { bd = d; best = j; }
        }
        const cld z = u;  // hqr returns exact conjugate pairs
        dn.erase(dn.begin() + (long)best);
        quads.push_back({-2.0L * z.real(), std::norm(z)});
    }
    std::sort(re.begin(), re.end());
    for (size_t i = 0; i + 1 < re.size(); i += 2) quads.push_back({-(re[i] + re[i + 1]), re[i] * re[i + 1]});
    if (re.size() & 1) quads.push_back({-re.back(), 0.0L});
    return true;
}

// Returns 0, or nonzero with *msg a printf format that takes the order, max(nb, na) - 1, as its one int
static int tf_to_sos(const double *b, int nb, const double *a, int na, std::vector<double> &sos, int *nsec_out, const char **msg)
{
    // normalise by a[0]; strip trailing zeros (roots at the origin contribute a unit factor)
    std::vector<long double> bb(b, b + nb), aa(a, a + na);
    for (auto &v : bb) v /= (long double)a[0];
    for (auto &v : aa) v /= (long double)a[0];
    while (bb.size() > 1 && bb.back() == 0.0L) bb.pop_back();
    while (aa.size() > 1 && aa.back() == 0.0L) aa.pop_back();
    int delay = 0;  // leading zeros of b = pure delays z^-delay
    while (bb.size() > 1 && bb.front() == 0.0L) { bb.erase(bb.begin()); ++delay; }
    const long double gain = bb.front();
    std::vector<std::pair<long double, long double>> zq, pq;
    if (gain != 0.0L) {
        std::vector<cld> zr;
        if (!(poly_roots(bb, zr) && quad_factors(zr, zq))) {
            *msg = "tf_create: could not factor the numerator into real second-order sections";
            return 1;
        }
    }
    std::vector<cld> pr;
    if (!(poly_roots(aa, pr) && quad_factors(pr, pq))) {
        *msg = "tf_create: could not factor the denominator into real second-order sections";
        return 2;
    }
    // delays become numerator factors z^-1 / z^-2
    std::vector<std::array<long double, 3>> num;
    for (auto &q : zq) num.push_back({1.0L, q.first, q.second});
    for (; delay >= 2; delay -= 2) num.push_back({0.0L, 0.0L, 1.0L});
    if (delay == 1) num.push_back({0.0L, 1.0L, 0.0L});
    const size_t ns = std::max<size_t>(std::max(num.size(), pq.size()), 1);
    if (ns > 12) {
        *msg = "tf_create: order %d needs more than 12 second-order sections";
        return 3;
    }
    // sections in order of increasing pole radius (quiet sections first), gain on the first
    std::sort(pq.begin(), pq.end(), [](const auto &x, const auto &y) { return x.second < y.second; });
    sos.assign(ns * 6, 0.0);
    for (size_t s = 0; s < ns; ++s) {
        std::array<long double, 3> nmr = s < num.size() ? num[s] : std::array<long double, 3>{1.0L, 0.0L, 0.0L};
        if (s == 0) for (auto &v : nmr) v *= gain;
        sos[6 * s + 0] = (double)nmr[0];
        sos[6 * s + 1] = (double)nmr[1];
        sos[6 * s + 2] = (double)nmr[2];
        sos[6 * s + 3] = 1.0;
        sos[6 * s + 4] = s < pq.size() ? (double)pq[s].first : 0.0;
        sos[6 * s + 5] = s < pq.size() ? (double)pq[s].second : 0.0;
    }
    *nsec_out = (int)ns;
    return 0;
}

// ---------------------------------------------------------------------------
// Biquad cascades as the handles hold them: 5 coefficients per section, b0 b1 b2 a1 a2 (a0 = 1).

// rows (b0, b1, b2, 1, a1, a2) of a scipy sos array -> coef; false when sos[:, 3] != 1
static inline bool sos_rows_to_coef(const double *sos, int nsec, std::vector<double> &coef)
{
    coef.resize((size_t)nsec * 5);
    for (int s = 0; s < nsec; ++s) {
        const double *q = sos + 6 * s;
        if (!(q[3] == 1.0)) return false;
        double *c = coef.data() + 5 * s;
        c[0] = q[0]; c[1] = q[1]; c[2] = q[2]; c[3] = q[4]; c[4] = q[5];
    }
    return true;
}

// v <- sections [s0, s1) applied to v (the reference's recursion: DF2T, from rest); reverse: section s1 - 1 first
static inline void df2t_run(const double *coef, int s0, int s1, std::vector<double> &v, bool reverse)
{
    for (int k = s0; k < s1; ++k) {
        const double *c = coef + 5 * (reverse ? s0 + s1 - 1 - k : k);
        double z0 = 0.0, z1 = 0.0;
        for (size_t i = 0; i < v.size(); ++i) {
            const double xn = v[i], xc = c[0] * xn + z0;
            z0 = c[1] * xn - c[3] * xc + z1;
            z1 = c[2] * xn - c[4] * xc;
            v[i] = xc;
        }
    }
}

// How far apart do two float64 evaluations of THIS cascade lie -- the reference's recursion with the sections as given and in reverse
// order (equal in exact arithmetic)?  A 40th-order Chebyshev design shows 1e-7 .. 1e-6 of its output; the scans (which combine chunk
// transitions instead of running the recursion) add 30 - 400 x that on such cascades (profiles/r05/iir_illcond.txt), which would carry
// them past the contract (1e-6 of the output for float32 signals, 1e-10 for float64 ones).  Returns diff / peak over 4096 samples of
// reproducible noise; 1.0 when that is not finite.
static inline double cascade_spread(const double *coef, int nsec)
{
    const int NH = 4096;
    std::vector<double> u(NH), v(NH);
    unsigned long long lcg = 0x9E3779B97F4A7C15ull;
    for (int i = 0; i < NH; ++i) {   // (sum of four uniforms: bell-shaped, unit-level, reproducible)
        double a = 0.0;
        for (int k = 0; k < 4; ++k) {
            lcg = lcg * 6364136223846793005ull + 1442695040888963407ull;
            a += (double)(lcg >> 11) / 9007199254740992.0 - 0.5;
        }
        u[i] = v[i] = a * 1.7320508075688772;
    }
    df2t_run(coef, 0, nsec, u, false);
    df2t_run(coef, 0, nsec, v, true);
    double peak = 0.0, diff = 0.0;
    for (int i = 0; i < NH; ++i) {
        peak = std::max(peak, std::fabs(u[i]));
        diff = std::max(diff, std::fabs(u[i] - v[i]));
    }
    return std::isfinite(diff) && peak > 0.0 ? diff / peak : 1.0;
}

// nsec sections in groups of at most `per`, as even as possible (10 -> 5 + 5)
static inline std::vector<int> group_sizes(int nsec, int per)
{
    const int ng = (nsec + per - 1) / per;
    std::vector<int> cnt((size_t)ng);
    for (int g = 0; g < ng; ++g) cnt[g] = nsec / ng + (g < nsec % ng ? 1 : 0);
    return cnt;
}

// Between two groups (of at most 8 sections) the signal is stored in the handle's precision.  For float32 handles that rounding (6e-8
// of the INTERMEDIATE's peak, then amplified by the rest of the cascade) must stay below the float32 contract on the output: with
// A = l1 norm of the impulse response up to a boundary, B = from it on, T = of the whole cascade, the boundary costs at most
// 6e-8 A B / T of the output's scale.  A Butterworth cascade has A B / T ~ 2; an order-17 Chebyshev in scipy's section order
// 170 (measured: 1e-5).  Returns the sum of A B / T over the boundaries.
static inline double boundary_cost(const double *coef, int nsec)
{
    // Cascades of more than 256 sections are not analysed (seconds of host work inside handle creation)
    if (nsec > 256) return 1e300;
    const int NH = 16384;
    auto l1 = [&](const std::vector<double> &v) { double a = 0.0; for (double q : v) a += std::fabs(q); return a; };
    std::vector<double> imp(NH, 0.0);
    imp[0] = 1.0;
    const std::vector<int> cnt = group_sizes(nsec, 8);
    const int ng8 = (int)cnt.size();
    // the boundaries' costs ADD UP (ng8 - 1 of them), so their sum is what is bounded; the l1 norms behind every boundary come from
    // ONE backward pass (sections commute: the tail from boundary g is the sections of group g applied to the tail from boundary
    // g + 1), the ones in front of it from one forward pass: O(nsec NH) in all.
    std::vector<int> first(ng8 + 1, 0);
    for (int g = 0; g < ng8; ++g) first[g + 1] = first[g] + cnt[g];
    std::vector<double> tail_l1(ng8 + 1, 0.0), v = imp;
    for (int g = ng8 - 1; g >= 1; --g) {   // v = impulse response of the sections [first[g], nsec)
        df2t_run(coef, first[g], first[g + 1], v, false);
        tail_l1[g] = l1(v);
    }
    df2t_run(coef, first[0], first[1], v, false);
    const double T = l1(v);
    std::vector<double> head = imp;
    double worst = 0.0;
    for (int g = 0; g + 1 < ng8; ++g) {
        df2t_run(coef, first[g], first[g + 1], head, false);
        worst += l1(head) * tail_l1[g + 1] / std::max(T, 1e-300);
    }
    return worst;
}

// unit-tail re-factorisation (see IirHandle): H_0' = H_0 * prod_{j>=1} b0_j,  H_k' = H_k / b0_k -- for cascades of at least two
// sections whose sections all have b2 == b0.  Rewrites coef in place and fills state_scale [2 nsec]; returns whether it applied
// (else both are untouched).
static inline bool unit_tail(double *coef, int nsec, std::vector<double> &state_scale)
{
    if (nsec < 2) return false;
    bool ok = true;
    for (int s = 0; s < nsec && ok; ++s) {
        const double *c = coef + 5 * s;
        ok = c[0] != 0.0 && std::isfinite(c[0]) && (s == 0 || std::fabs(c[2] / c[0] - 1.0) <= 1e-13);
    }
    if (!ok) return false;
    std::vector<long double> tail((size_t)nsec + 1, 1.0L);  // tail[k] = prod_{j>=k} b0_j
    for (int s = nsec - 1; s >= 0; --s) tail[s] = tail[s + 1] * (long double)coef[5 * s];
    for (int s = 0; s < nsec && ok; ++s) ok = std::isfinite((double)tail[s]) && tail[s] != 0.0L;
    if (!ok) return false;
    state_scale.resize((size_t)2 * nsec);
    for (int s = 0; s < nsec; ++s) {
        double *c = coef + 5 * s;
        if (s == 0) {
            for (int k = 0; k < 3; ++k) c[k] = (double)((long double)c[k] * tail[1]);
        } else {
            const long double b0 = c[0];
            c[1] = (double)((long double)c[1] / b0);
            c[0] = 1.0;
            c[2] = 1.0;
        }
        state_scale[2 * s] = state_scale[2 * s + 1] = (double)tail[s + 1];
    }
    return true;
}

}  // namespace skdsp
